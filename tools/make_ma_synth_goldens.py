#!/usr/bin/env python3
"""Generate tests/golden/ma_synth/ by running the REAL reference's `ma` (oracle/_ref/ma, built by oracle/Makefile.ref) on the
synthetic cases of tests/maln_synth.py: -f 41 and -f 5 under both consensus codes, -f 4 under code 1.  Runs only where the reference
can be built; the recorded outputs are committed, the generated .maln texts are not (the tests rebuild them from the seeds).

  tests/golden/ma_synth/runs.json        {case: {seed, records, sha256 of the .maln text from its MALN_NAS line on}}, "keys": the runs
  tests/golden/ma_synth/hashes.json      {"<case>.<run key>": {sha256, bytes}} of every output
  tests/golden/ma_synth/outputs.json.gz  {case: {run key: stdout}} of every case but the big ones (maln_synth.BIG_CASES) ...
  tests/golden/ma_synth/<case>.f41c<code>.gz   ... whose -f 41 tables are files of their own (their other outputs are pinned by
                                         hashes.json and rebuilt from the table's reading in tests/maln_synth.py)
"""
import gzip
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import maln_synth as ms  # noqa: E402

MA = os.path.join(ROOT, "oracle", "_ref", "ma")
OUT = os.path.join(ROOT, "tests", "golden", "ma_synth")
INIT_NUM_ALN_SEQS = 16000          # src/params.h:69: the deep case must make read_ma grow its record array


def run_reference(path, key):
    fmt, code = key[1:].split("c")
    return subprocess.run([MA, "-M", path, "-f", fmt, "-c", code], check=True, stdout=subprocess.PIPE).stdout


def gz_write(path, data):
    with open(path, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0, filename="") as z:
        z.write(data)


def main():
    t0 = time.time()
    subprocess.run(["make", "-s", "-f", "oracle/Makefile.ref"], check=True, cwd=ROOT)
    shutil.rmtree(OUT, ignore_errors=True)
    os.makedirs(OUT)
    tmp = tempfile.mkdtemp()
    runs, hashes, outputs = {"keys": list(ms.RUN_KEYS)}, {}, {}
    for name, c in ms.CASES.items():
        m = ms.make_case(name)
        text = ms.write_maln(m)
        path = os.path.join(tmp, name + ".maln")
        with open(path, "w", encoding="latin1") as f:
            f.write(ms.MA_HEADER + text)
        runs[name] = {"seed": c["seed"], "records": len(m.rec), "sha256": hashlib.sha256(text.encode("latin1")).hexdigest()}
        small = {}
        for key in ms.RUN_KEYS:
            out = run_reference(path, key)
            hashes[f"{name}.{key}"] = {"sha256": hashlib.sha256(out).hexdigest(), "bytes": len(out)}
            if name not in ms.BIG_CASES:
                small[key] = out.decode("latin1")
            elif key.startswith("f41"):
                gz_write(os.path.join(OUT, f"{name}.{key}.gz"), out)
        if name in ms.BIG_CASES:
            # the reference read every record: each of them is in the coverage of some column
            table = gzip.open(os.path.join(OUT, f"{name}.f41c1.gz")).read().decode().split("\n")
            deepest = max(int(line.split()[3]) for line in table if line)
            print(f"{name}: {len(m.rec)} records (INIT_NUM_ALN_SEQS {INIT_NUM_ALN_SEQS}), deepest column {deepest}")
        else:
            outputs[name] = small
        os.remove(path)
    shutil.rmtree(tmp)

    def one_line_each(d):                                  # a JSON object, one entry per line
        return "{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(d[k], sort_keys=True)}" for k in sorted(d)) + "\n}\n"

    with open(os.path.join(OUT, "runs.json"), "w") as f:
        f.write(one_line_each(runs))
    with open(os.path.join(OUT, "hashes.json"), "w") as f:
        f.write(one_line_each(hashes))
    gz_write(os.path.join(OUT, "outputs.json.gz"), json.dumps(outputs, sort_keys=True).encode())
    print("ma_synth goldens:", len(ms.CASES), "cases,", len(hashes), "runs, %.1f s" % (time.time() - t0))


if __name__ == "__main__":
    main()
