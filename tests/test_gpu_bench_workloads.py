"""The bytes bench.py times, against the oracle.

bench.py's headline runs make_workload(1, 1 000 000, seed=1) -- and configs[2] make_workload(2, 1 000 000, seed=3) -- to the fixed
point and prints `certificate`: sha256 of the consensus and of every read's (score, as, ae).  Here the SAME workloads are built by
the same function and run the same way (bench.Pipeline.step = mia_hip_iterate), and

* 4 000 sampled reads go through every realignment of the run in the oracle, read by read (the plan finishes four reads in five
  without any DP on this data: this is the check of that shortcut on the benched bytes, not on another seed);
* 50 000 reads of the batch run three iterations side by side with the oracle in a context of their own: every read's result, the
  dropped marks, all ten tally words of every column, ref->gaps, the consensus;
* the digests equal tests/golden/bench_certificates.json -- what BENCH_r06.json's line must show as well (HIP-made);
* EVERY read after steps 1 and 2, and the consensus of step 1, digest to what the reference's own loop computed for the same
  reads (tests/golden/bench_certificates_ref.json, tools/make_ref_certificates.py); a mismatch is narrowed to a block of 8 192
  reads and those go through the oracle to name the reads (tests/ref_certificates.py);
* the first 200 000 reads of each workload, in a context of their own, run to the fixed point: consensus and every read after
  every iteration against the reference's single-process run of the same reads -- cull, tally and consensus over a six-figure
  read set against reference-made output.
configs[3] and configs[4] at their bench seeds and sizes: test_gpu_config3.py, test_gpu_config4_full.py (same file of digests)."""
import json
import os

import numpy as np
import pytest

import ref_certificates as rcert
from conftest import GOLDEN
from oracle_sample import PushedOracle, check_subset_iterations

pytestmark = pytest.mark.gpu

PINNED = json.load(open(os.path.join(GOLDEN, "bench_certificates.json")))
REF = rcert.load()
_workloads = {}


def workload(cfg, seed, n=1_000_000):
    import bench
    if cfg not in _workloads:
        _workloads[cfg] = bench.make_workload(cfg, n, seed)
    return _workloads[cfg]


def pinned(cert, key):
    want = PINNED[key]
    got = {k: cert[k] for k in ("consensus_sha256", "alignments_sha256", "consensus_len")}
    assert got == {k: want[k] for k in got}, (key, got, want)


@pytest.mark.parametrize("cfg,seed", [(1, 1), (2, 3)])
def test_benched_workload_against_oracle(cfg, seed, oracle):
    import bench
    import mia_amd
    n = 1_000_000
    w = workload(cfg, seed)
    hip = mia_amd.MiaHip(0)
    pipe = bench.Pipeline(hip, w)
    refs, als, cur = [], [], w["ref"]
    for _ in range(12):
        nxt = pipe.step(cur)
        refs.append(cur)
        if len(als) < 3:
            als.append(hip.alignments())
        if nxt == cur:
            break
        cur = nxt
    assert nxt == cur and 2 <= len(refs) <= 6
    cert = bench.certificate(hip, nxt, True)
    hip.close()
    pinned(cert, "cfg%d" % cfg)
    assert PINNED["cfg%d" % cfg]["iterations_to_convergence"] == len(refs)
    # every read, against what the reference's own loop computed for it
    ref = REF["cfg%d" % cfg]
    rcert.check_consensus(refs[1], ref["consensus_sha256"], ref["consensus_len"], "cfg%d step 1" % cfg)
    for it in (1, 2):
        rerun = rcert.oracle_rerun(oracle, refs[:it], True, w["matrix_file"], w["stored"], w["rc"], w["as_"], w["ae"])
        rcert.check_alignments(als[it - 1], ref, it, "cfg%d" % cfg, rerun)
    # the sample, through the run's own sequence of references
    pick = np.sort(np.random.default_rng(100 + cfg).choice(n, 4000, replace=False))
    po = PushedOracle(oracle, w["ref"], True, w["matrix_file"], w["stored"][pick], w["rc"][pick], w["as_"][pick], w["ae"][pick])
    for it, (ref, al) in enumerate(zip(refs, als), 1):
        po.iterate(ref)
        o = po.alignments()
        for k in range(3):
            bad = np.nonzero(al[k][pick] != o[k])[0]
            assert len(bad) == 0, (cfg, it, k, len(bad), pick[bad[:5]].tolist())
    po.close()
    # a subset with everything the consensus is made of
    sub = np.sort(np.random.default_rng(200 + cfg).choice(n, 50_000, replace=False))
    first = tuple(a[sub] for a in als[0])
    done, _ = check_subset_iterations(mia_amd, oracle, w["ref"], True, w["matrix_file"], w["pssm"], w["stored"][sub], w["rc"][sub], np.ones(len(sub), np.uint8),
                                      w["as_"][sub], w["ae"][sub], iters=3, expect_first=first)
    assert done >= 2


@pytest.mark.parametrize("cfg,seed", [(1, 1), (2, 3)])
def test_prefix_to_the_fixed_point_against_reference(cfg, seed, oracle):
    import bench
    import mia_amd
    ref = REF["cfg%d_prefix" % cfg]
    P = ref["reads"]
    w = workload(cfg, seed)
    wp = dict(w, n=P, stored=w["stored"][:P], rc=w["rc"][:P], as_=w["as_"][:P], ae=w["ae"][:P], offsets=w["offsets"][:P + 1], lens=w["lens"][:P])
    hip = mia_amd.MiaHip(0)
    pipe = bench.Pipeline(hip, wp)
    refs, cons, als, cur = [], [], [], w["ref"]
    for _ in range(12):
        nxt = pipe.step(cur)
        refs.append(cur)
        cons.append(nxt)
        als.append(hip.alignments())
        if nxt == cur:
            break
        cur = nxt
    hip.close()
    assert nxt == cur
    # the reference's driver stops after the first iteration that returns the consensus it was given as well
    assert len(refs) == ref["iterations_run"], (len(refs), ref["iterations_run"])
    for it in range(1, len(refs) + 1):
        want = ref["iterations"][str(it)]
        rcert.check_consensus(cons[it - 1], want["consensus_sha256"], want["consensus_len"], "cfg%d prefix iteration %d" % (cfg, it))
        rerun = rcert.oracle_rerun(oracle, refs[:it], True, w["matrix_file"], wp["stored"], wp["rc"], wp["as_"], wp["ae"])
        rcert.check_alignments(als[it - 1], ref, it, "cfg%d prefix" % cfg, rerun)
