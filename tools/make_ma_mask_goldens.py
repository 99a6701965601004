#!/usr/bin/env python3
"""Generate tests/golden/ma_mask/outputs.json.gz with the REAL reference's `ma` (oracle/_ref/ma, built by oracle/Makefile.ref), so that
the end mask of ma_hip -E / -x is held to what the reference itself reads out of the masked files, not only to tests/ma_mask_ref.py.  A
trimmed record is still a legal .maln record, so no new .maln is committed: the inputs are reference-written files the repository
already holds (tests/ma_mask_goldens.py, INPUTS).  Runs only where the reference can be built.

  outputs.json.gz   "files": per input and setting "<n5>_<n3>_<trim|N|Nss>" the reference's `ma -f 41 -c 1`, `ma -f 5` and `ma -f 1` on
                    the file the RESTATEMENT has masked (tests/ma_mask_ref.py), each the text itself or, above 200 000 bytes,
                    {"sha256": .., "bytes": ..}; and "counts", the restatement's hist and scalars

Nothing is written unless, by the restatement alone, the fixtures together show every rare path (tests/ma_mask_goldens.py,
rare_paths): without that a mask that ignored one of them could pass.
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
import ma_mask_goldens as mg  # noqa: E402
import ma_mask_ref as ref  # noqa: E402
import maln_synth as ms  # noqa: E402

MA = os.path.join(ROOT, "oracle", "_ref", "ma")
OUT = os.path.join(ROOT, "tests", "golden", "ma_mask")


def run(cmd, cwd):
    r = subprocess.run(cmd, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if r.returncode != 0:
        sys.exit("%s failed: exit %d: %r" % (" ".join(cmd), r.returncode, r.stderr[-300:]))
    return r.stdout


def main():
    subprocess.run(["make", "-s", "-f", "oracle/Makefile.ref"], check=True, cwd=ROOT)
    masks = mg.all_masks()
    missing = mg.rare_paths(masks)
    if missing:
        sys.exit("the inputs are no fixture: they lack " + ", ".join(missing))
    outputs = {"files": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for name in mg.INPUTS:
            outputs["files"][name] = {}
            for s in ref.SETTINGS:
                m, got = masks[name][ref.tag(*s)]
                with open(os.path.join(tmp, "masked.maln"), "w", encoding="latin1") as f:
                    f.write(ms.MA_HEADER + ms.write_maln(got.maln))
                entry = {"counts": got.counts()}
                for key, args in mg.RUNS:
                    out = run([MA, "-M", "masked.maln"] + args, tmp)
                    entry[key] = out.decode("latin1") if len(out) <= 200000 else {"sha256": hashlib.sha256(out).hexdigest(), "bytes": len(out)}
                outputs["files"][name][ref.tag(*s)] = entry
                c = entry["counts"]
                print("%s %s: %d of %d records kept, %d pairs dropped, %d stripped, %d columns counted" %
                      (name, ref.tag(*s), c["n_kept"], len(m.rec), c["pairs_dropped"], c["stripped"], sum(c["hist"])))
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "outputs.json.gz")
    with open(path, "wb") as raw, gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as f:
        f.write((json.dumps(outputs, sort_keys=True, separators=(",", ":")) + "\n").encode())
    print("outputs.json.gz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
