#!/usr/bin/env python3
"""Generate tests/golden/ma_collapse/outputs.json.gz with the REAL reference's ma (oracle/_ref/ma, built by oracle/Makefile.ref): what
it prints for the files the RESTATEMENT of the duplicate consensus (tests/ma_collapse_ref.py) has collapsed, so that ma_hip -u -j is
held to the reference's reading of those files and not to ma_hip's own.  Runs only where the reference can be built.  No .maln is
written into the repository.

  "sets"    for tests/golden/ma_dedup/reads_a.maln.1.gz and reads_b.maln.1.gz (the reference's own `mia -c -n -H 1` runs) and tolerance 0
            and 2: the reference's `ma -f 41 -c 1`, `ma -f 5` and `ma -f 1` on the collapsed file, each the text itself or, above 200 000
            bytes, {"sha256": .., "bytes": ..}, and the restatement's hist (72 numbers)
  "cases"   the same for every case of tests/maln_collapse_cases.py

The vote is ma_hip's: a dropped record does not vote.  The tool refuses to write unless, by the restatement alone, the set shows
every path (see the assertions at the end of main)."""
import gzip
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ma_collapse_ref as ref  # noqa: E402
import maln_collapse_cases as cc  # noqa: E402
import maln_synth as ms  # noqa: E402

MA = os.path.join(ROOT, "oracle", "_ref", "ma")
OUT = os.path.join(ROOT, "tests", "golden", "ma_collapse")
SETS = ("reads_a", "reads_b")
FORMATS = (("f41c1", ["-f", "41", "-c", "1"]), ("f5", ["-f", "5"]), ("f1", ["-f", "1"]))


def run(cmd, cwd):
    r = subprocess.run(cmd, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if r.returncode != 0:
        sys.exit("%s failed: exit %d: %r" % (" ".join(cmd), r.returncode, r.stderr[-300:]))
    return r.stdout


def record(m, t, tmp):
    """the reference's outputs for the file the restatement collapsed, and what the restatement counted on the way"""
    vote = ref.not_dropped(m)
    new, _members, hist = ref.collapse(m, t, vote)
    with open(os.path.join(tmp, "new.maln"), "w", encoding="latin1") as f:
        f.write(ms.MA_HEADER + ms.write_maln(new))
    out = {"hist": [int(x) for x in hist.reshape(-1)]}
    for tag, args in FORMATS:
        text = run([MA, "-M", "new.maln"] + args, tmp)
        out[tag] = text.decode("latin1") if len(text) <= 200000 else {"sha256": hashlib.sha256(text).hexdigest(), "bytes": len(text)}
    return out


def paths(m, t):
    """what the restatement met in this file: counts of the paths the set has to show"""
    vote = ref.not_dropped(m)
    keep, _rep, clusters, _totals = ref.clusters_of(m.rec, m.L, t)
    seen = dict(to_base=0, to_gap=0, to_N=0, kept_tie=0, base_over_gap=0, edge_gap=0, no_vote_letter=0, dropped_voter=0, half_reps=0, sizes=set())
    for best, mols in clusters:
        if len(mols) < 2:
            continue
        seen["sizes"].add(len(mols))
        voters = [mol for mol in mols if vote[mol[5][0]]]
        seen["dropped_voter"] += len(mols) - len(voters)
        for R in best[5]:
            r = m.rec[R]
            seen["half_reps"] += r["seg"] in ("f", "b")
            n = r["end"] - r["start"] + 1
            for c in range(n):
                counts = {}
                for mol in voters:
                    ch = ref.vote_at(m.rec, mol, r["start"] + c)
                    if ch is None:
                        continue
                    if ch.upper() not in ref.CLASSES:
                        seen["no_vote_letter"] += 1
                        continue
                    seen["edge_gap"] += ch == "-" and c in (0, n - 1)
                    counts[ch.upper()] = counts.get(ch.upper(), 0) + 1
                new, _voted, _split, what = ref.decide(counts, r["seq"][c], c in (0, n - 1))
                live = {k: v for k, v in counts.items() if not (k == "-" and c in (0, n - 1))}
                tie = bool(live) and sum(1 for v in live.values() if v == max(live.values())) > 1
                seen["kept_tie"] += tie and what is None
                seen["to_base"] += what == ref.TO_BASE
                seen["to_gap"] += what == ref.TO_GAP
                seen["to_N"] += what == ref.TO_N
                seen["base_over_gap"] += what == ref.TO_BASE and r["seq"][c] == "-"
    return seen


def main():
    subprocess.run(["make", "-s", "-f", "oracle/Makefile.ref"], check=True, cwd=ROOT)
    os.makedirs(OUT, exist_ok=True)
    outputs = {"sets": {}, "cases": {}}
    total = dict(to_base=0, kept_tie=0, half_reps=0)
    synth = dict(to_gap=0, base_over_gap=0, to_N=0, edge_gap=0, no_vote_letter=0, dropped_voter=0)
    with tempfile.TemporaryDirectory() as tmp:
        for name in SETS:
            with gzip.open(os.path.join(ROOT, "tests", "golden", "ma_dedup", name + ".maln.1.gz"), "rt", encoding="latin1") as f:
                m = ms.parse_maln(f.read().split("\n", 1)[1])
            outputs["sets"][name] = {str(t): record(m, t, tmp) for t in (0, 2)}
            seen = paths(m, 0)
            print(name, {k: (sorted(v) if isinstance(v, set) else v) for k, v in seen.items()})
            for k in total:
                total[k] += seen[k]
        for name in cc.CASES:
            m = cc.case(name)
            outputs["cases"][name] = {str(t): record(m, t, tmp) for t in (0, 2)}
            seen = paths(m, 0)
            for k in synth:
                synth[k] += seen[k]
    print("reference-written inputs:", total, "synthetic cases:", synth)
    # by the restatement alone: the two reference-written inputs together change at least 5 columns to another base, keep own on at
    # least 20 ties and have representatives that are halves of split reads; the synthetic cases show every other path
    assert total["to_base"] >= 5 and total["kept_tie"] >= 20 and total["half_reps"] >= 1, total
    assert all(v >= 1 for v in synth.values()), synth
    data = (json.dumps(outputs, sort_keys=True, separators=(",", ":")) + "\n").encode()
    path = os.path.join(OUT, "outputs.json.gz")
    with open(path, "wb") as raw, gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as f:      # no time stamp, no name: the same bytes for the same content
        f.write(data)
    print("outputs.json.gz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
