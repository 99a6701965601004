#!/usr/bin/env python3
"""Generate tests/golden/ma_ends/ by running the REAL reference's `ma -f 3` (oracle/_ref/ma, built by oracle/Makefile.ref) on the cases
tests/test_ma_ends_cpu.py names: columns 5-8 of its per-column table -- the fragments that start and that end on each reference column,
per strand (col_print_cons, src/map_align.c:761-849) -- are what ties the true ends of tests/ma_ends_ref.py to the reference.  Runs only
where the reference can be built; the recorded counts are committed, the generated .maln texts are not (the tests rebuild them from
the seeds).

  tests/golden/ma_ends/f3_ends.json   {case: {"records", "sha256" of the .maln text the reference read, from its MALN_NAS line on,
                                       "rows": the table's rows on reference columns, "ends": {column (0-based): [forward starts,
                                       reverse starts, forward ends, reverse ends]}, the columns where one of them is not zero}}
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import maln_ace_cases as mc  # noqa: E402
import maln_ends_cases as ec  # noqa: E402
import maln_synth as ms  # noqa: E402

MA = os.path.join(ROOT, "oracle", "_ref", "ma")
OUT = os.path.join(ROOT, "tests", "golden", "ma_ends")
NAMES = tuple("ends:" + n for n in ec.CASES) + ("ace:shapes", "ace:column300") + tuple("ace:" + n for n in mc.FIXTURES) + ("synth:deep",)
LAST_HEADER = "# 8. Number of fragments on reverse strand that end here"


def case_text(name):
    """the text the reference reads for a case, from its MALN_NAS line on"""
    kind, key = name.split(":", 1)
    if kind == "ends":
        return ms.write_maln(ec.for_the_reference(ec.make_case(key)))
    return mc.case_text(key) if kind == "ace" else ms.write_maln(ms.make_case(key))


def table_ends(stdout):
    """(rows on reference columns, {column: [c5, c6, c7, c8]} where not all zero).  An insert column (reference character '-') repeats
    the counts of a reference column and is left out."""
    lines = stdout.decode("latin1").split("\n")
    at = lines.index(LAST_HEADER) + 1
    rows, ends = 0, {}
    for ln in lines[at:]:
        if not ln:
            continue
        f = ln.split("\t")
        assert len(f) == 8, ln
        if f[1] == "-":
            continue
        rows += 1
        four = [int(x) for x in f[4:8]]
        if any(four):
            col = int(f[3]) - 1
            assert col not in ends, (col, ln)
            ends[col] = four
    return rows, ends


def main():
    subprocess.run(["make", "-s", "-f", "oracle/Makefile.ref"], check=True, cwd=ROOT)
    os.makedirs(OUT, exist_ok=True)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name in NAMES:
            text = case_text(name)
            path = os.path.join(tmp, "in.maln")
            with open(path, "w", encoding="latin1") as f:
                f.write(ms.MA_HEADER + text)
            r = subprocess.run([MA, "-M", path, "-f", "3"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            if r.returncode != 0:
                sys.exit(f"the reference's ma -f 3 failed on {name}: exit {r.returncode}: {r.stderr[-300:]!r}")
            rows, ends = table_ends(r.stdout)
            out[name] = {"records": int(text.split("\n", 1)[0].split()[1]), "sha256": hashlib.sha256(text.encode("latin1")).hexdigest(), "rows": rows,
                         "ends": {str(c): ends[c] for c in sorted(ends)}}
    with open(os.path.join(OUT, "f3_ends.json"), "w") as f:
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(out[k], sort_keys=True)}" for k in sorted(out)) + "\n}\n")
    print("ma_ends goldens:", len(out), "cases,", sum(len(c["ends"]) for c in out.values()), "columns with an end,",
          os.path.getsize(os.path.join(OUT, "f3_ends.json")), "bytes")


if __name__ == "__main__":
    main()
