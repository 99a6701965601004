#!/usr/bin/env python3
"""Generate tests/golden/ma_pmd/outputs.json.gz with the REAL reference's `ma` (oracle/_ref/ma, built by oracle/Makefile.ref), so that
the damage score filter of ma_hip -L is held to what the reference's own `ma` reads out of the reduced files, not only to
tests/ma_pmd_ref.py.  Runs only where the reference can be built.  No new .maln is committed: the inputs are the two files the
reference's `mia` wrote for the deaminated-fragment filter, tests/golden/ma_damage/reads_a.maln.1.gz and reads_b.maln.1.gz.

  outputs.json.gz       "sets": per input and setting "<T>_<ds|ss>" the reference's `ma -f 41 -c 1` and `ma -f 5` on the file the
                        RESTATEMENT has reduced (tests/ma_pmd_ref.py, with its own model table at the default parameters), each the
                        text itself or, above 200 000 bytes, {"sha256": .., "bytes": ..}; "kept", the records that stay; "molecules",
                        [[forward kept, forward removed], [reverse kept, reverse removed]]; "range", the smallest and the largest
                        molecule score in units of 2^-16 nat

Nothing is written unless, by the restatement alone, at (3, ds) every strand x kept / removed class holds at least 20 molecules in both
files, and each file has at least 4 split molecules whose two record scores have opposite signs: without that the filter could pass by
keeping everything or nothing, or by scoring halves apart.
"""
import gzip
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ma_dedup_ref  # noqa: E402
import ma_pmd_ref as ref  # noqa: E402
import maln_damage_cases as dc  # noqa: E402
import maln_synth as ms  # noqa: E402

MA = os.path.join(ROOT, "oracle", "_ref", "ma")
IN = os.path.join(ROOT, "tests", "golden", "ma_damage")
OUT = os.path.join(ROOT, "tests", "golden", "ma_pmd")
SETTINGS = ((3, False), (0, False), (5, False), (3, True), (8, False))
MIN_CLASS, MIN_OPPOSITE = 20, 4


def run(cmd, cwd):
    r = subprocess.run(cmd, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if r.returncode != 0:
        sys.exit("%s failed: exit %d: %r" % (" ".join(cmd), r.returncode, r.stderr[-300:]))
    return r.stdout


def tag(nat, ss):
    return "%d_%s" % (nat, "ss" if ss else "ds")


def classes(m, mate, mol, keep):
    """[[forward kept, forward removed], [reverse kept, reverse removed]] in molecules"""
    out = [[0, 0], [0, 0]]
    for r, rec in enumerate(m.rec):
        if mate[r] < 0 or r < mate[r]:
            out[1 if rec["rc"] else 0][0 if keep[r] else 1] += 1
    return out


def main():
    subprocess.run(["make", "-s", "-f", "oracle/Makefile.ref"], check=True, cwd=ROOT)
    outputs = {"sets": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for name in dc.READ_SETS:
            with gzip.open(os.path.join(IN, name + ".maln.1.gz"), "rb") as f:
                m = ms.parse_maln(f.read().decode("latin1").split("\n", 1)[1])
            mate, ev = ma_dedup_ref.pair_halves(m.rec), ref.events(m)
            outputs["sets"][name] = {}
            for nat, ss in SETTINGS:
                rec, mol, keep, _hist, _n, n_kept, _o = ref.score(m, ref.model_table(ss=ss), ref.threshold_of(nat), None, mate, ev=ev)
                cls = classes(m, mate, mol, keep)
                if (nat, ss) == (3, False):
                    opposite = sum(1 for r in range(len(m.rec)) if mate[r] > r and int(rec[r]) * int(rec[mate[r]]) < 0)
                    print("%s: molecules kept / removed %s, %d split molecules with halves of opposite sign, scores %.2f .. %.2f nat" %
                          (name, cls, opposite, mol.min() / 65536, mol.max() / 65536))
                    if min(min(c) for c in cls) < MIN_CLASS or opposite < MIN_OPPOSITE:
                        sys.exit("%s is no fixture for the damage score" % name)
                assert 0 < n_kept < len(keep), (name, nat, ss)
                with open(os.path.join(tmp, "less.maln"), "w", encoding="latin1") as f:
                    f.write(ms.MA_HEADER + ms.write_maln(ref.reduce(m, keep)))
                entry = {"kept": n_kept, "molecules": cls, "range": [int(mol.min()), int(mol.max())]}
                for key, args in (("f41c1", ["-f", "41", "-c", "1"]), ("f5", ["-f", "5"])):
                    got = run([MA, "-M", "less.maln"] + args, tmp)
                    entry[key] = got.decode("latin1") if len(got) <= 200000 else {"sha256": hashlib.sha256(got).hexdigest(), "bytes": len(got)}
                outputs["sets"][name][tag(nat, ss)] = entry
                print("  %s: %d of %d records stay" % (tag(nat, ss), n_kept, len(keep)))
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "outputs.json.gz"), "wb") as raw, gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as f:
        f.write((json.dumps(outputs, sort_keys=True, separators=(",", ":")) + "\n").encode())
    print("outputs.json.gz", os.path.getsize(os.path.join(OUT, "outputs.json.gz")), "bytes")


if __name__ == "__main__":
    main()
