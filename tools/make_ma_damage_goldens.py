#!/usr/bin/env python3
"""Generate tests/golden/ma_damage/ with the REAL reference (oracle/_ref/mia and oracle/_ref/ma, built by oracle/Makefile.ref), so that
the deaminated-fragment filter of ma_hip -D is held to files the reference wrote and to what the reference's own `ma` reads out of
the reduced files, not only to tests/ma_damage_ref.py.  Runs only where the reference can be built.

  <set>.maln.1.gz       the reference's `mia -c -n -H 1 -s ancient.submat.txt` on a seeded read set with simulated damage
                        (tests/maln_damage_cases.py, read_set), as written (first line replaced: it carries a date)
  outputs.json.gz       "seeds": the seed of either set; "sets": per set and reduction "<N>_<mode>_<ds|ss>" the reference's
                        `ma -f 41 -c 1` and `ma -f 5` on the file the RESTATEMENT has reduced (tests/ma_damage_ref.py), each the
                        text itself or, above 200 000 bytes, {"sha256": .., "bytes": ..}; and "kept", the records that stay

A seed is taken only if, by the restatement alone, on either strand every class at N = 3 (no hit, 5' only, 3' only, both) holds at
least five molecules, and one split molecule hits in its front half only and one in its back half only: without that the filter
could pass by keeping everything or nothing.
"""
import gzip
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ma_damage_ref as ref  # noqa: E402
import ma_dedup_ref  # noqa: E402
import maln_damage_cases as dc  # noqa: E402
import maln_synth as ms  # noqa: E402

MIA = os.path.join(ROOT, "oracle", "_ref", "mia")
MA = os.path.join(ROOT, "oracle", "_ref", "ma")
OUT = os.path.join(ROOT, "tests", "golden", "ma_damage")
MATRIX = os.path.join(ROOT, "tests", "golden", "ancient.submat.txt")
REDUCTIONS = ((3, "any", False), (1, "5", False), (2, "both", False), (3, "3", True), (15, "any", False), (1, "3", False))
FIRST_SEED = {"reads_a": 9600, "reads_b": 9700}


def run(cmd, cwd):
    r = subprocess.run(cmd, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if r.returncode != 0:
        sys.exit("%s failed: exit %d: %r" % (" ".join(cmd), r.returncode, r.stderr[-300:]))
    return r.stdout


def write_gz(name, data):
    """gzip without a time stamp or a file name: the same bytes for the same content"""
    with open(os.path.join(OUT, name), "wb") as raw, gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as f:
        f.write(data)
    print(name, os.path.getsize(os.path.join(OUT, name)), "bytes")


def tag(n_pos, mode, ss):
    return "%d_%s_%s" % (n_pos, mode, "ss" if ss else "ds")


def fit(m):
    """is the file a fixture: the classes at N = 3 on either strand, the split molecules"""
    pos5, pos3, _keep, hist, _n, _k, _o = ref.damage(m, 3, "any", False)
    for strand in (0, 1):
        h = hist[strand]
        none, both = h[0, 0] + h[0, 4:].sum() + h[4:, 0].sum() + h[4:, 4:].sum(), h[1:4, 1:4].sum()
        only5, only3 = h[1:4, 0].sum() + h[1:4, 4:].sum(), h[0, 1:4].sum() + h[4:, 1:4].sum()
        if min(none, both, only5, only3) < 5:
            return False
    mate = ma_dedup_ref.pair_halves(m.rec)
    front_only = back_only = 0
    for r, rec in enumerate(m.rec):
        if rec["seg"] == "f" and mate[r] >= 0:
            b = int(mate[r])
            hit_f, hit_b = bool(pos5[r] or pos3[r]), bool(pos5[b] or pos3[b])
            front_only += hit_f and not hit_b
            back_only += hit_b and not hit_f
    return front_only >= 1 and back_only >= 1


def main():
    subprocess.run(["make", "-s", "-f", "oracle/Makefile.ref"], check=True, cwd=ROOT)
    os.makedirs(OUT, exist_ok=True)
    outputs = {"seeds": {}, "sets": {}}
    for name in dc.READ_SETS:
        with tempfile.TemporaryDirectory() as tmp:
            shutil.copy(MATRIX, os.path.join(tmp, "ancient.submat.txt"))
            for seed in range(FIRST_SEED[name], FIRST_SEED[name] + 50):
                fa_ref, fa_reads = dc.read_set(name, seed)
                with open(os.path.join(tmp, "ref.fa"), "w") as f:
                    f.write(fa_ref)
                with open(os.path.join(tmp, "reads.fa"), "w") as f:
                    f.write(fa_reads)
                run([MIA, "-r", "ref.fa", "-f", "reads.fa", "-c", "-n", "-H", "1", "-s", "ancient.submat.txt", "-m", "out"], tmp)
                with open(os.path.join(tmp, "out.1"), encoding="latin1") as f:
                    text = f.read().split("\n", 1)[1]
                m = ms.parse_maln(text)
                if fit(m):
                    break
                print("%s: seed %d is no fixture" % (name, seed))
            else:
                sys.exit("%s: no seed gives a fixture" % name)
            split = sum(1 for r in m.rec if r["seg"] == "f")
            print("%s: seed %d, %d records, %d front halves, strands %s" % (name, seed, len(m.rec), split, sorted({r["rc"] for r in m.rec})))
            outputs["seeds"][name] = seed
            write_gz(name + ".maln.1.gz", (ms.MA_HEADER + text).encode("latin1"))
            outputs["sets"][name] = {}
            for n_pos, mode, ss in REDUCTIONS:
                keep = ref.damage(m, n_pos, mode, ss)[2]
                assert 0 < keep.sum() < len(keep), (name, n_pos, mode, ss)
                with open(os.path.join(tmp, "less.maln"), "w", encoding="latin1") as f:
                    f.write(ms.MA_HEADER + ms.write_maln(ref.reduce(m, keep)))
                entry = {"kept": int(keep.sum())}
                for key, args in (("f41c1", ["-f", "41", "-c", "1"]), ("f5", ["-f", "5"])):
                    got = run([MA, "-M", "less.maln"] + args, tmp)
                    entry[key] = got.decode("latin1") if len(got) <= 200000 else {"sha256": hashlib.sha256(got).hexdigest(), "bytes": len(got)}
                outputs["sets"][name][tag(n_pos, mode, ss)] = entry
                print("  %s: %d of %d records stay" % (tag(n_pos, mode, ss), int(keep.sum()), len(keep)))
    write_gz("outputs.json.gz", (json.dumps(outputs, sort_keys=True, separators=(",", ":")) + "\n").encode())


if __name__ == "__main__":
    main()
