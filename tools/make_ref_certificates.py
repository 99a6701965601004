#!/usr/bin/env python3
"""Build box, no GPU: what the REFERENCE computes for every read of the workloads bench.py times, written to
tests/golden/bench_certificates_ref.json.  The other side of tests/golden/bench_certificates.json (HIP-made,
tools/make_bench_certificates.py): tests/test_bench_certificates_cpu.py holds the two files against each other, the GPU tests
hold every read of a run against this one (tests/ref_certificates.py).  Never imported by a test.

The reference's own per-iteration loop is oracle/_ref/ref_iter_driver (oracle/ref_iter_driver.c linked against the reference's
objects by oracle/Makefile.ref); with a dump argument it writes the consensus and every read's (score, as, ae) after each
iteration.  The cost per read of one process grows with its read store (200 000 reads take 17 minutes), so

  chunks   cfg1 (1 M, seed 1), cfg2 (1 M, seed 3), cfg3 (10 M paired, seed 4) -- the make_workload calls of
           make_bench_certificates.py -- are cut into contiguous chunks of CHUNK[cfg] reads, each chunk one driver process of two
           iterations, at most min(cores, free memory / 5 GB) at a time.  Every chunk's consensus after iteration 1 and after
           iteration 2 must be ONE string for the whole workload (else iteration 2 of the chunks would not be iteration 2 of
           the batch: the script stops).  Per iteration: sha256 over all reads' score, as, ae (int32 LE, the three arrays one
           after the other: bench.certificate's layout) and one 16-hex digest per block of BLOCK reads in the same layout.
  prefix   the first PREFIX reads of cfg1 and of cfg2 in ONE process each, to the fixed point (2 iterations; 3 when the second
           still moved the consensus): consensus and alignment digests after every iteration -- cull, tally and consensus over
           a six-figure read set.
  proof    the prefix run's per-read lines must equal the chunked run's for the same reads, in iterations 1 and 2: per-read
           results depend on the read, the reference string and the matrix, not on the read's company ("chunk_independent").
cfg4 (100 kb linear reference) is not covered; the golden says why.

Dumps are parsed into <scratch>/<target>/*.npz as they finish, so a broken-off run resumes where it stopped.
usage: python3 tools/make_ref_certificates.py [--scratch DIR] [--jobs N] [target ...] [--assemble]
       targets: cfg1 cfg2 cfg3 prefix1 prefix2 (default: all, the long single processes first); --assemble writes the golden from finished targets"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools")); sys.path.insert(0, os.path.join(ROOT, "tests"))

DRIVER = os.path.join(ROOT, "oracle", "_ref", "ref_iter_driver")
OUT = os.path.join(ROOT, "tests", "golden", "bench_certificates_ref.json")
WORKLOADS = {1: (1_000_000, 1), 2: (1_000_000, 3), 3: (10_000_000, 4)}       # make_bench_certificates.py WORKLOADS, less cfg4
CHUNK = {1: 50_000, 2: 50_000, 3: 25_000}       # the cost per read grows with the process's read store: the 10 M workload gets the smaller chunks
BLOCK = 8192
PREFIX = 200_000
GB_PER_PROCESS = 5
CFG4_NOTE = ("make_workload(4, 5000000, seed=5): a linear reference's thin ends make a chunk's consensus depend on the chunk, so a chunk's "
             "iteration 2 is not the batch's, and one process for 5 M reads of 150 bp against 100 kb is out of reach (200 000 reads of 100 bp "
             "against 16.6 kb take 17 minutes and the cost per read grows with the read store; cfg4's own cost was not measured); "
             "cfg4 stays oracle-sampled (tests/test_gpu_config4_full.py)")


def digest(score, as_, ae):
    h = hashlib.sha256()
    for x in (score, as_, ae):
        h.update(np.ascontiguousarray(x, dtype="<i4").tobytes())
    return h.hexdigest()


def block_digests(score, as_, ae, block=BLOCK):
    return [digest(score[i:i + block], as_[i:i + block], ae[i:i + block])[:16] for i in range(0, len(score), block)]


def max_jobs():
    free_gb = 0
    with open("/proc/meminfo") as f:
        for line in f:
            if line.startswith("MemAvailable:"):
                free_gb = int(line.split()[1]) / 1e6
    return max(1, min(os.cpu_count() or 1, int(free_gb // GB_PER_PROCESS)))


def parse_dump(path, n):
    """-> ([consensus after iteration k], int32 [iterations, n, 3])"""
    cons, rows = [], []
    with open(path) as f:
        text = f.read()
    for part in text.split("I ")[1:]:
        head, _, body = part.partition("\n")
        k, c = head.split()
        assert int(k) == len(cons) + 1, (path, k)
        cons.append(c)
        r = np.array(body.replace("R", " ").split(), dtype=np.int64).reshape(-1, 3)
        assert len(r) == n and body.count("R") == n, (path, k, len(r), n)
        assert np.abs(r).max() < 2 ** 31
        rows.append(r.astype(np.int32))
    return cons, np.stack(rows)


def run_driver(w, lo, hi, iters, work, ref_fa, keep_dump=False):
    """reads [lo, hi) of w in one driver process; -> (cons list, results, seconds wall, peak RSS in KB)"""
    tag = "%d_%d_%d" % (lo, hi, iters)
    npz = os.path.join(work, tag + ".npz")
    if os.path.exists(npz):
        z = np.load(npz)
        return [str(c) for c in z["cons"]], z["al"], float(z["wall"]), int(z["rss_kb"])
    reads, dump = os.path.join(work, tag + ".reads.txt"), os.path.join(work, tag + ".dump.txt")
    with open(reads, "w") as f:                                              # the lines of bench.cpu_baseline
        for i in range(lo, hi):
            f.write(f"{int(w['rc'][i])} {int(w['as_'][i])} {int(w['ae'][i])} {w['stored'][i].tobytes().decode()}\n")
    matrix = os.path.join(ROOT, "tests", "golden", w["matrix_file"]) if w["matrix_file"] else "flat"
    t0 = time.time()
    p = subprocess.Popen([DRIVER, ref_fa, reads, "1" if w["circular"] else "0", matrix, str(iters), dump], stdout=subprocess.DEVNULL)
    rss_kb = 0                  # VmHWM of the driver itself (a waited child's ru_maxrss carries this process's own size across the exec)
    while p.poll() is None:
        try:
            with open("/proc/%d/status" % p.pid) as f:
                rss_kb = max([rss_kb] + [int(line.split()[1]) for line in f if line.startswith("VmHWM:")])
        except OSError:
            pass
        time.sleep(0.5)
    wall = time.time() - t0
    if p.returncode != 0:
        raise RuntimeError("ref_iter_driver failed (%d) on reads [%d, %d)" % (p.returncode, lo, hi))
    cons, al = parse_dump(dump, hi - lo)
    assert len(cons) == iters
    np.savez(npz + ".tmp.npz", cons=np.array(cons), al=al, wall=wall, rss_kb=rss_kb)
    os.replace(npz + ".tmp.npz", npz)
    os.remove(reads)
    if not keep_dump:
        os.remove(dump)
    return cons, al, wall, rss_kb


def workload(cfg, scratch):
    import bench
    import gen_data
    n, seed = WORKLOADS[cfg]
    w = bench.make_workload(cfg, n, seed)
    ref_fa = os.path.join(scratch, "ref_cfg%d.fa" % cfg)
    gen_data.write_fasta(ref_fa, "ref", w["ref"])
    return w, ref_fa, "make_workload(%d, %d, seed=%d)" % (cfg, n, seed)


def chunked(cfg, scratch, pool, jobs):
    """submits the chunks to the pool; the returned function waits for them and writes the target's result"""
    w, ref_fa, name = workload(cfg, scratch)
    n = w["n"]
    work = os.path.join(scratch, "cfg%d" % cfg)
    os.makedirs(work, exist_ok=True)
    cuts = [(lo, min(lo + CHUNK[cfg], n)) for lo in range(0, n, CHUNK[cfg])]
    t0 = time.time()
    futures = [pool.submit(run_driver, w, lo, hi, 2, work, ref_fa) for lo, hi in cuts]
    return lambda: chunked_finish(cfg, scratch, jobs, w, name, work, cuts, futures, t0)


def chunked_finish(cfg, scratch, jobs, w, name, work, cuts, futures, t0):
    n = w["n"]
    res = [f.result() for f in futures]
    wall = time.time() - t0
    S = res[0][0][0]
    for (lo, hi), (cons, _, _, _) in zip(cuts, res):                      # one string, both iterations, every chunk: no papering over
        for k, c in enumerate(cons, 1):
            if c != S:
                raise SystemExit("cfg%d: chunk [%d, %d) consensus after iteration %d (sha256 %s, %d bp) is not the workload's (%s, %d bp)"
                                 % (cfg, lo, hi, k, hashlib.sha256(c.encode()).hexdigest()[:12], len(c), hashlib.sha256(S.encode()).hexdigest()[:12], len(S)))
    if S != w["plain_ref"]:
        raise SystemExit("cfg%d: the chunks agree on a consensus that is not the individual the reads were drawn from" % cfg)
    al = np.concatenate([r[1] for r in res], axis=1)                        # [2, n, 3]
    np.save(os.path.join(work, "all.npy"), al[:, :PREFIX])                  # for the proof of chunk independence
    out = {"workload": name, "reads": n, "chunk": CHUNK[cfg], "block": BLOCK, "made_by": "oracle/_ref/ref_iter_driver",
           "consensus_sha256": hashlib.sha256(S.encode()).hexdigest(), "consensus_len": len(S), "iterations": {}}
    cost = {"cost": {"processes": jobs, "wall_s": round(wall, 1), "chunk_cpu_s_sum": round(sum(r[2] for r in res), 1),
                    "chunk_wall_s_max": round(max(r[2] for r in res), 1), "peak_rss_gb_per_process": round(max(r[3] for r in res) / 1e6, 2)}}
    for k in (1, 2):
        sc, a, e = (np.ascontiguousarray(al[k - 1, :, j]) for j in range(3))
        out["iterations"][str(k)] = {"alignments_sha256": digest(sc, a, e), "blocks": block_digests(sc, a, e)}
    json.dump(out, open(os.path.join(scratch, "result_cfg%d.json" % cfg), "w"), indent=1, sort_keys=True)
    print("cfg%d" % cfg, {k: v for k, v in out.items() if k != "iterations"}, cost, flush=True)


def prefix(cfg, scratch, pool):
    w, ref_fa, name = workload(cfg, scratch)
    work = os.path.join(scratch, "prefix%d" % cfg)
    os.makedirs(work, exist_ok=True)
    return pool.submit(prefix_run, cfg, scratch, w, ref_fa, name, work).result


def prefix_run(cfg, scratch, w, ref_fa, name, work):
    cons, al, wall, rss = run_driver(w, 0, PREFIX, 2, work, ref_fa, keep_dump=True)
    if cons[1] != cons[0]:                                                  # not yet a fixed point: one more round, and say so
        cons, al, wall, rss = run_driver(w, 0, PREFIX, 3, work, ref_fa, keep_dump=True)
        if cons[2] != cons[1]:
            raise SystemExit("prefix of cfg%d: no fixed point in 3 iterations" % cfg)
    np.save(os.path.join(work, "all.npy"), al)
    out = {"workload": name + "[:%d]" % PREFIX, "reads": PREFIX, "made_by": "oracle/_ref/ref_iter_driver", "iterations_run": len(cons),
           "iterations": {}}
    cost = {"cost": {"processes": 1, "wall_s": round(wall, 1), "peak_rss_gb_per_process": round(rss / 1e6, 2)}}
    for k, c in enumerate(cons, 1):
        sc, a, e = (np.ascontiguousarray(al[k - 1, :, j]) for j in range(3))
        out["iterations"][str(k)] = {"consensus_sha256": hashlib.sha256(c.encode()).hexdigest(), "consensus_len": len(c),
                                     "alignments_sha256": digest(sc, a, e), "blocks": block_digests(sc, a, e)}
    json.dump(out, open(os.path.join(scratch, "result_prefix%d.json" % cfg), "w"), indent=1, sort_keys=True)
    print("prefix%d" % cfg, {k: v for k, v in out.items() if k != "iterations"}, cost, flush=True)


def assemble(scratch):
    out = {"cfg4": {"not_covered": CFG4_NOTE}, "chunk_independent": True, "block": BLOCK, "made_by": "oracle/_ref/ref_iter_driver"}
    for cfg in (1, 2, 3):
        out["cfg%d" % cfg] = json.load(open(os.path.join(scratch, "result_cfg%d.json" % cfg)))
        out["cfg%d" % cfg].pop("cost", None)                                # digests and counts only: the cost goes to the log
    for cfg in (1, 2):
        p = json.load(open(os.path.join(scratch, "result_prefix%d.json" % cfg)))
        p.pop("cost", None)
        whole = np.load(os.path.join(scratch, "cfg%d" % cfg, "all.npy"))
        alone = np.load(os.path.join(scratch, "prefix%d" % cfg, "all.npy"))
        for k in (0, 1):                                                    # the licence for the chunked runs
            bad = np.nonzero((whole[k] != alone[k]).any(axis=1))[0]
            if len(bad):
                raise SystemExit("cfg%d iteration %d: %d of the first %d reads differ between one process and the chunks, first %s: %s alone, %s chunked"
                                 % (cfg, k + 1, len(bad), PREFIX, bad[:5].tolist(), alone[k][bad[:5]].tolist(), whole[k][bad[:5]].tolist()))
        out["cfg%d_prefix" % cfg] = p
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    json.dump(out, open(OUT, "w"), indent=None, sort_keys=True, separators=(",", ":"))
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("targets", nargs="*")
    ap.add_argument("--scratch", default=os.path.join(tempfile.gettempdir(), "mia_ref_certificates"))
    ap.add_argument("--jobs", type=int, default=0)
    ap.add_argument("--assemble", action="store_true")
    a = ap.parse_args()
    if os.path.abspath(a.scratch).startswith(ROOT + os.sep):
        raise SystemExit("--scratch must lie outside the repository")
    if not os.path.exists(DRIVER):
        raise SystemExit("oracle/_ref/ref_iter_driver missing: make -f oracle/Makefile.ref")
    os.makedirs(a.scratch, exist_ok=True)
    # one pool for everything, longest single processes first: the two prefix runs, then the chunks
    targets = a.targets or ([] if a.assemble else ["prefix1", "prefix2", "cfg3", "cfg1", "cfg2"])
    jobs = min(a.jobs, max_jobs()) if a.jobs else max_jobs()
    with ThreadPoolExecutor(jobs) as pool:
        waits = [chunked(int(t[3:]), a.scratch, pool, jobs) if t.startswith("cfg") else prefix(int(t[6:]), a.scratch, pool) for t in targets]
        for wait in waits:
            wait()
    if a.assemble or not a.targets:
        assemble(a.scratch)
