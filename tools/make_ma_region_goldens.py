#!/usr/bin/env python3
"""Generate tests/golden/ma_region/ by running the REAL reference's `ma` (oracle/_ref/ma, built by oracle/Makefile.ref)
on every committed tests/golden/maln/*.[0-9]: the clustalw and line reports (-f 1, -f 2, consensus codes 1 and 2, and
no -f at all) and the region view (-f 6, -f 61) over a fixed list of regions.  Runs only where the reference can be
built; the recorded outputs are committed so that a machine without it can replay them.

  tests/golden/ma_region/runs.json        every recorded run: "common" {run key: the arguments behind `-M <file>`} of the runs
                                          every file gets, "regions" {maln name: {tag: -R argument or null}} -- each region
                                          is two runs, "f6.<tag>" and "f61.<tag>" (expand_runs below)
  tests/golden/ma_region/outputs.json.gz  {maln name: {run key: stdout}} of the runs whose output is at most 40 KB (the
                                          region views of near-identical assemblies repeat each other: 1 MB of text, gzip)
  tests/golden/ma_region/hashes.json      {"<maln>.<run key>": {sha256, bytes}} of the larger ones

tools/make_goldens.py (everything else under tests/golden) is left as it is.
"""
import glob
import gzip
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RB = os.path.join(ROOT, "oracle", "_ref")
G = os.path.join(ROOT, "tests", "golden")
MA_HEADER = "/* map_alignment [V1.0] */ golden\n"   # line 1 of a .maln carries a timestamp and is not stored
MIN_INSERT_REGIONS = 3


def maln_shape(path):
    """(reference length, ref->gaps) of a .maln"""
    length = None
    for line in open(path):
        if length is None and line.startswith("LEN "):
            length = int(line.split()[1])
        if line.startswith("GAPS"):
            return length, [int(x) for x in line.split()[1:]]
    raise ValueError(path)


def regions(name, length, gaps):
    """[(tag, -R argument or None, has insert columns)]: the fixed list, and for the indel_* / fix_* files a region that holds
    a column with gaps > 0 and one that starts exactly on it"""
    out = [("Rnone", None), ("R1_60", "1:60"), ("Rend", f"{max(1, length - 99)}:{length}"), ("Rpast", f"{length - 10}:{length + 50}"),
           ("Rbeyond", f"{length + 10}:{length + 60}"), ("Rswap", "200:100"), ("Rhalf", "50")]
    if name.startswith(("indel_", "fix_")):
        cols = [p for p, g in enumerate(gaps) if g > 0 and p > 0]
        if cols:
            q = cols[0] + 1                                   # 1-based
            out.append(("Rins", f"{max(1, q - 10)}:{min(length, q + 10)}"))
            out.append(("Rins_start", f"{q}:{min(length, q + 20)}"))
    res = []
    for tag, arg in out:
        a, b = 90, 109                                        # parse_region / print_region, to know what the region holds
        if arg is not None:
            parts = arg.split(":")
            a = int(parts[0])
            if len(parts) > 1:
                b = int(parts[1])
            if a > b:
                a = b
        a, b = max(a, 1), min(b, length)
        res.append((tag, arg, any(g > 0 for g in gaps[a - 1:b])))
    return res


COMMON = {"default": [], "f6.C": ["-f", "6", "-C", "-R", "1:60"], "f61.I": ["-f", "61", "-I", "my_assembly"]}
COMMON.update({f"f{fmt}c{code}": ["-f", str(fmt), "-c", str(code)] for fmt in (1, 2) for code in (1, 2)})


def expand_runs(common, region_args):
    """{run key: arguments} of one .maln"""
    runs = dict(common)
    for tag, arg in region_args.items():
        for fmt in (6, 61):
            runs[f"f{fmt}.{tag}"] = ["-f", str(fmt)] + (["-R", arg] if arg is not None else [])
    return runs


def main():
    subprocess.run(["make", "-s", "-f", "oracle/Makefile.ref"], check=True, cwd=ROOT)
    out_dir = os.path.join(G, "ma_region")
    shutil.rmtree(out_dir, ignore_errors=True)
    os.makedirs(out_dir)
    tmp = tempfile.mkdtemp()
    all_regions, hashes, outputs, insert_regions, n_runs = {}, {}, {}, 0, 0
    for path in sorted(glob.glob(os.path.join(G, "maln", "*.[0-9]"))):
        name = os.path.basename(path)
        full = os.path.join(tmp, name)
        with open(full, "w") as f:
            f.write(MA_HEADER + open(path).read())
        length, gaps = maln_shape(path)
        reg = regions(name, length, gaps)
        insert_regions += sum(1 for _, _, has_ins in reg if has_ins)
        all_regions[name] = {tag: arg for tag, arg, _ in reg}
        runs = expand_runs(COMMON, all_regions[name])
        small = {}
        for key, args in runs.items():
            out = subprocess.run([os.path.join(RB, "ma"), "-M", full] + args, check=True, stdout=subprocess.PIPE).stdout
            if len(out) <= 40 * 1024:
                small[key] = out.decode("latin1")
            else:
                hashes[f"{name}.{key}"] = {"sha256": hashlib.sha256(out).hexdigest(), "bytes": len(out)}
        n_runs += len(runs)
        outputs[name] = small
    shutil.rmtree(tmp)
    if insert_regions < MIN_INSERT_REGIONS:
        sys.exit(f"only {insert_regions} regions with insert columns: the file set does not exercise them")

    def one_line_each(d):                                  # a JSON object, one entry per line
        return "{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(d[k], sort_keys=True)}" for k in sorted(d)) + "\n}\n"

    with open(os.path.join(out_dir, "runs.json"), "w") as f:
        f.write(one_line_each({"common": COMMON, "regions": all_regions}))
    with open(os.path.join(out_dir, "hashes.json"), "w") as f:
        f.write(one_line_each(hashes))
    with open(os.path.join(out_dir, "outputs.json.gz"), "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0, filename="") as z:
        z.write(json.dumps(outputs, sort_keys=True).encode())
    print("ma_region goldens:", n_runs, "runs,", len(hashes), "hashed,", insert_regions, "regions with insert columns")


if __name__ == "__main__":
    main()
