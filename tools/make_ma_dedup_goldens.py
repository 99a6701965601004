#!/usr/bin/env python3
"""Generate tests/golden/ma_dedup/ with the REAL reference (oracle/_ref/mia and oracle/_ref/ma, built by oracle/Makefile.ref): what
`mia -u` keeps of two seeded read sets (tests/maln_dedup_cases.py, read_set), so that the duplicate filter of ma_hip -u is held to the
reference end to end and not only to tests/ma_dedup_ref.py.  Runs only where the reference can be built.

  <set>.maln.1.gz       the reference's `mia -c -n -H 1` on the set, without -u (first line replaced: it carries a date)
  runs.json.gz          per set and run ("plain", "u": -H 1; "plain_cut", "u_cut": the default score cut) the records' fields
                        [ID, RC, START, END, SEG, SCORE, DR, INS_POS pairs] in file order and the GAPS line
  outputs.json.gz       "sets": per set the reference's `ma -f 41 -c 1`, `-f 5 -c 1` and `-f 5 -c 2` on its own `mia -c -n -H 1 -u` run;
                        "cases": for every case of tests/maln_dedup_cases.py and tolerance 0 and 2 the reference's `ma -f 41 -c 1` and
                        `ma -f 5` on the file the RESTATEMENT has reduced (tests/ma_dedup_ref.py), each the text itself or, above
                        200 000 bytes, {"sha256": .., "bytes": ..}
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
import ma_dedup_ref as ref  # noqa: E402
import maln_dedup_cases as dc  # noqa: E402
import maln_synth as ms  # noqa: E402

MIA = os.path.join(ROOT, "oracle", "_ref", "mia")
MA = os.path.join(ROOT, "oracle", "_ref", "ma")
OUT = os.path.join(ROOT, "tests", "golden", "ma_dedup")
RUNS = {"plain": ["-H", "1"], "u": ["-H", "1", "-u"], "plain_cut": [], "u_cut": ["-u"]}


def run(cmd, cwd):
    r = subprocess.run(cmd, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if r.returncode != 0:
        sys.exit("%s failed: exit %d: %r" % (" ".join(cmd), r.returncode, r.stderr[-300:]))
    return r.stdout


def fields(m):
    return [[r["id"], r["rc"], r["start"], r["end"], r["seg"], r["score"], r["dr"], [list(x) for x in r["ins"]]] for r in m.rec]


def write_gz(name, data):
    """gzip without a time stamp or a file name: the same bytes for the same content"""
    with open(os.path.join(OUT, name), "wb") as raw, gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as f:
        f.write(data)
    print(name, os.path.getsize(os.path.join(OUT, name)), "bytes")


def dump(obj):
    return (json.dumps(obj, sort_keys=True, separators=(",", ":")) + "\n").encode()


def main():
    subprocess.run(["make", "-s", "-f", "oracle/Makefile.ref"], check=True, cwd=ROOT)
    os.makedirs(OUT, exist_ok=True)
    out, outputs, falls = {}, {"sets": {}}, 0
    for name in dc.READ_SETS:
        fa_ref, fa_reads = dc.read_set(name)
        with tempfile.TemporaryDirectory() as tmp:
            with open(os.path.join(tmp, "ref.fa"), "w") as f:
                f.write(fa_ref)
            with open(os.path.join(tmp, "reads.fa"), "w") as f:
                f.write(fa_reads)
            out[name], text = {}, {}
            for key, flags in RUNS.items():
                run([MIA, "-r", "ref.fa", "-f", "reads.fa", "-c", "-n", "-m", key] + flags, tmp)
                with open(os.path.join(tmp, key + ".1"), encoding="latin1") as f:
                    text[key] = f.read().split("\n", 1)[1]
                m = ms.parse_maln(text[key])
                out[name][key] = {"records": fields(m), "gaps": m.gaps.tolist()}
            plain, u = ms.parse_maln(text["plain"]), ms.parse_maln(text["u"])
            pairs = sum(1 for r in plain.rec if r["seg"] == "f")
            strands = {r["rc"] for r in plain.rec}
            fell = int(((plain.gaps > 0) & (u.gaps < plain.gaps)).sum())
            assert pairs >= 20 and strands == {0, 1} and len(u.rec) < len(plain.rec), (name, pairs, strands)
            # the restatement at tolerance 0 must already give the -u run: a read set on which it does not is no fixture
            keep = ref.dedup(plain.rec, plain.L, 0)[0]
            mine = ref.reduce(plain, keep)
            key5 = lambda r: (r["rc"], r["start"], r["end"], r["seg"], r["score"])
            assert sorted(map(key5, mine.rec)) == sorted(map(key5, u.rec)), name
            assert mine.gaps.tolist() == u.gaps.tolist(), name
            write_gz(name + ".maln.1.gz", (ms.MA_HEADER + text["plain"]).encode("latin1"))
            outputs["sets"][name] = {tag: run([MA, "-M", "u.1"] + args, tmp).decode("latin1")
                                     for tag, args in (("f41c1", ["-f", "41", "-c", "1"]), ("f5c1", ["-f", "5", "-c", "1"]), ("f5c2", ["-f", "5", "-c", "2"]))}
            print("%s: %d -> %d records, %d split pairs, GAPS falls on %d columns" % (name, len(plain.rec), len(u.rec), pairs, fell))
            falls = falls + fell
    assert falls >= 1, "no column where GAPS falls"
    write_gz("runs.json.gz", dump(out))
    outputs["cases"] = cases()
    write_gz("outputs.json.gz", dump(outputs))


def cases():
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name in dc.CASES:
            m = dc.case(name)
            out[name] = {}
            for t in (0, 2):
                less = ref.reduce(m, ref.dedup(m.rec, m.L, t)[0])
                with open(os.path.join(tmp, "less.maln"), "w", encoding="latin1") as f:
                    f.write(ms.MA_HEADER + ms.write_maln(less))
                out[name][str(t)] = {}
                for tag, args in (("f41c1", ["-f", "41", "-c", "1"]), ("f5", ["-f", "5"])):
                    text = run([MA, "-M", "less.maln"] + args, tmp)
                    out[name][str(t)][tag] = text.decode("latin1") if len(text) <= 200000 else {"sha256": hashlib.sha256(text).hexdigest(), "bytes": len(text)}
    return out


if __name__ == "__main__":
    main()
