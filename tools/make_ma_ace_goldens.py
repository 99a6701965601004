#!/usr/bin/env python3
"""Generate tests/golden/ma_ace/ by running the REAL reference's `ma` (oracle/_ref/ma, built by oracle/Makefile.ref) on the cases of
tests/maln_ace_cases.py: the ACE export (-f 7) under both consensus codes and with -I, and the rewrite (-m).  Runs only where the
reference can be built; the recorded outputs are committed, the generated .maln texts are not (the tests rebuild them from the seeds).

  tests/golden/ma_ace/runs.json        {case: {records, sha256 of the .maln text from its MALN_NAS line on}}, "runs": the arguments
  tests/golden/ma_ace/hashes.json      {"<case>.<run>.stdout" / "<case>.<run>.file": {sha256, bytes}} of every output; the file -m
                                       wrote counts from its second line on (the first carries the date)
  tests/golden/ma_ace/outputs.json.gz  {case: {run: {"stdout": .., "file": ..}}}: the full text of every output of at most TEXT_LIMIT bytes
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
import maln_ace_cases as mc  # noqa: E402
import maln_synth as ms  # noqa: E402

MA = os.path.join(ROOT, "oracle", "_ref", "ma")
OUT = os.path.join(ROOT, "tests", "golden", "ma_ace")
TEXT_LIMIT = 200_000


def gz_write(path, data):
    with open(path, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0, filename="") as z:
        z.write(data)


def main():
    subprocess.run(["make", "-s", "-f", "oracle/Makefile.ref"], check=True, cwd=ROOT)
    shutil.rmtree(OUT, ignore_errors=True)
    os.makedirs(OUT)
    tmp = tempfile.mkdtemp()
    runs, hashes, outputs = {"runs": mc.RUNS}, {}, {}
    for name in mc.CASES:
        text = mc.case_text(name)
        path = os.path.join(tmp, name + ".maln")
        with open(path, "w", encoding="latin1") as f:
            f.write(ms.MA_HEADER + text)
        runs[name] = {"records": int(text.split("\n", 1)[0].split()[1]), "sha256": hashlib.sha256(text.encode("latin1")).hexdigest()}
        outputs[name] = {}
        for key, args in mc.RUNS.items():
            written = os.path.join(tmp, name + "." + key + ".out")
            r = subprocess.run([MA, "-M", path] + [written if a == "OUT" else a for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            if r.returncode != 0:
                sys.exit(f"the reference's ma failed on {name} {key}: exit {r.returncode}: {r.stderr[-300:]!r}")
            got = {"stdout": r.stdout}
            if "OUT" in args:
                with open(written, "rb") as f:
                    got["file"] = f.read().split(b"\n", 1)[1]
                os.remove(written)
            outputs[name][key] = {}
            for what, data in got.items():
                hashes[f"{name}.{key}.{what}"] = {"sha256": hashlib.sha256(data).hexdigest(), "bytes": len(data)}
                if len(data) <= TEXT_LIMIT:
                    outputs[name][key][what] = data.decode("latin1")
        os.remove(path)
    shutil.rmtree(tmp)

    def one_line_each(d):                                  # a JSON object, one entry per line
        return "{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(d[k], sort_keys=True)}" for k in sorted(d)) + "\n}\n"

    with open(os.path.join(OUT, "runs.json"), "w") as f:
        f.write(one_line_each(runs))
    with open(os.path.join(OUT, "hashes.json"), "w") as f:
        f.write(one_line_each(hashes))
    gz_write(os.path.join(OUT, "outputs.json.gz"), json.dumps(outputs, sort_keys=True).encode())
    print("ma_ace goldens:", len(mc.CASES), "cases,", len(hashes), "outputs,", sum(len(o) for c in outputs.values() for o in c.values()), "in full,",
          os.path.getsize(os.path.join(OUT, "outputs.json.gz")), "bytes of outputs.json.gz")


if __name__ == "__main__":
    main()
