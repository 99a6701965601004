"""The duplicate consensus (ma_hip -u -j, -f 98) without a GPU.  tests/ma_collapse_ref.py restates the rule of DESIGN.md ("Duplicate
consensus") as plain loops; here it is held to results written out by hand and, at tolerance 0, to a plain group-by with
collections.Counter.  The code the kernels run per lane (csrc/ma_collapse_body.h) is compiled for the host into
tests/ma_collapse_driver.cpp, with -fsanitize=address,undefined where g++ has that runtime, and run as a program of its own: its staged
form (plan, count per chunk, decide) must agree with its own serial walk and with the restatement for every case and tolerance.  The
files the restatement collapses are the ones the compiled reference's ma read for tests/golden/ma_collapse."""
import collections
import gzip
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

import ma_collapse_ref as ref
import ma_dedup_ref as ddref
import maln_collapse_cases as cc
import maln_synth as ms
from conftest import ROOT

_want = {}


def want(name, t):
    if (name, t) not in _want:
        m = cc.case(name)
        _want[name, t] = ref.collapse_records(m, t, ref.not_dropped(m))
    return _want[name, t]


def test_the_hand_results():
    m = cc.case("hand")
    assert [r["id"] for r in m.rec] == ["a_rep", "a_1", "a_2", "b_0", "b_rep", "c_0", "c_rep", "d_0", "d_1", "d_rep", "e_0", "e_1", "e_rep", "single"]
    out, keep, members, hist, n_collapsed, n_changed, totals = ref.collapse_records(m, 0, ref.not_dropped(m))
    assert keep.tolist() == [1, 0, 0, 0, 1, 0, 1, 0, 0, 1, 0, 0, 1, 1]
    assert members.tolist() == [3, 0, 0, 0, 2, 0, 2, 0, 0, 3, 0, 0, 3, 0]
    # a: column 5 T>A twice against the representative's T; the lower-case c stays; a_2's '-' on the last column does not count
    # b: C against A ties and own C stays; the one T replaces own N.  c: the dropped representative does not vote, c_0 decides N and R
    # d: three classes tie, own A is one.  e: the dropped representative's A is in neither tied class: N
    assert [r["seq"] for r in out] == ["GTAcGAAC", "GTACGAAC", "GCACGAA-", "GATTAC", "GCTTAC", "ACAGA", "ACAGA", "TTTTT", "TGTTT", "TATTT", "CCCCC", "CGCCC", "CNCCC",
                                       "ACGT"]
    assert [r["num_inputs"] for r in out] == [3, 1, 1, 1, 2, 1, 1, 1, 1, 3, 1, 1, 2, 1]
    by_hand = np.zeros((2, 6, 6), np.int64)
    by_hand[0, 1] = [3, 8 + 5 + 5, 2 + 1 + 1, 1, 0, 1]        # forward, three molecules: a, d, e
    by_hand[1, 0] = [2, 6 + 5, 1, 1 + 2, 0, 0]                # reverse, two molecules: b, c
    assert np.array_equal(hist, by_hand) and (n_collapsed, n_changed) == (5, 5) and totals == (14, 6, 0)
    new = ref.collapse(m, 0, ref.not_dropped(m))[0]
    assert [(r["id"], r["seq"], r["num_inputs"]) for r in new.rec] == [("a_rep", "GTAcGAAC", 3), ("b_rep", "GCTTAC", 2), ("c_rep", "ACAGA", 1), ("d_rep", "TATTT", 3),
                                                                    ("e_rep", "CNCCC", 2), ("single", "ACGT", 1)]
    # everyone votes: c's own N and R are no votes, so nothing else changes there; e's A makes three classes tie and stays
    every = ref.collapse_records(m, 0, None)[0]
    assert [r["seq"] for r in every][6] == "ACAGA" and [r["seq"] for r in every][12] == "CACCC" and every[12]["num_inputs"] == 3
    assert ref.report(m, 0, ref.not_dropped(m)).split("\n")[0] == "# ma_hip duplicate consensus: 14 molecules, 6 clusters, 5 collapsed, 0 orphans, tolerance 0"


def test_the_votes_case_shows_every_decision():
    m = cc.case("votes")
    out = want("votes", 0)[0]
    by_id = {r["id"]: (r, o) for r, o in zip(m.rec, out)}
    g, g2 = by_id["g_rep"]
    assert g2["seq"][4] == "-" and g["seq"][4] != "-"                    # '-' wins in the middle
    assert g["seq"][6] == "-" and g2["seq"][6] == by_id["g_1"][0]["seq"][6]      # a base replaces the representative's '-'
    assert g2["seq"][0] == g["seq"][0] and g2["seq"][11] == g["seq"][11]  # two '-' against one base at the edges: not counted
    t, t2 = by_id["t_rep"]
    assert t2["seq"][3] == t["seq"][3] and t2["seq"][5] == "N"           # a tie that keeps own, a tie that gives N
    assert t2["seq"][7] == t["seq"][7] and t["seq"][7].islower()         # lower case survives where it wins
    assert t2["seq"][8] == by_id["t_1"][0]["seq"][8] and t2["seq"][8].isupper()
    assert t2["seq"][9] == t["seq"][9] and t2["seq"][10] == t["seq"][10]  # N and IUPAC voters are no votes
    e, e2 = by_id["e_rep"]
    assert e["seq"][0] == "-" and e2["seq"][0] == by_id["e_2"][0]["seq"][0]


@pytest.mark.parametrize("name", cc.CASES)
def test_tolerance_0_is_a_group_by_with_a_counter(name):
    m = cc.case(name)
    vote = ref.not_dropped(m)
    out, keep, members, hist = want(name, 0)[:4]
    assert np.array_equal(keep, ddref.dedup(m.rec, m.L, 0)[0])          # which records survive does not change
    groups = ddref.group_by(m.rec, m.L)
    sizes = collections.Counter()
    for (rc, _a, _e), mols in groups.items():
        if len(mols) < 2:
            for x in mols:
                assert all(out[r]["seq"] == m.rec[r]["seq"] and out[r]["num_inputs"] == m.rec[r]["num_inputs"] and members[r] == 0 for r in x[5])
            continue
        sizes[rc, ref.size_bin(len(mols))] += 1
        best = max(mols, key=lambda x: (x[3], -x[4]))
        voters = [x for x in mols if vote[x[5][0]]]
        for x in mols:
            for r in x[5]:
                assert members[r] == (len(mols) if x is best else 0)
                if x is not best:
                    assert out[r]["seq"] == m.rec[r]["seq"]
        for R in best[5]:
            r = m.rec[R]
            n = r["end"] - r["start"] + 1
            for c in range(n):
                p = r["start"] + c
                tally = collections.Counter()
                for x in voters:
                    chars = [m.rec[q]["seq"][p - m.rec[q]["start"]].upper() for q in x[5] if m.rec[q]["start"] <= p <= m.rec[q]["end"]][:1]
                    tally.update(ch for ch in chars if ch in "ACGT" or (ch == "-" and 0 < c < n - 1))
                own, new = r["seq"][c], out[R]["seq"][c]
                if not tally:
                    assert new == own
                    continue
                ranked = tally.most_common()
                ahead = [ch for ch, k in ranked if k == ranked[0][1]]
                if len(ahead) == 1:
                    assert new == (own if ahead[0] == own.upper() else ahead[0]), (name, R, c)
                else:
                    assert new == (own if own.upper() in ahead else "N"), (name, R, c)
            assert out[R]["seq"][n:] == r["seq"][n:]
    assert {k: int(v) for k, v in np.ndenumerate(hist[:, :, 0]) if v} == dict(sizes)


def test_the_report_of_an_empty_file():
    text = ref.report(cc.case("empty"), 0)
    assert text.count("\n") == 14 and text.split("\n")[2] == "2\t+\t0\t0\t0\t0\t0\t0" and text.split("\n")[13] == "17+\t-\t0\t0\t0\t0\t0\t0"


def sanitizer_flags(tmp):
    """-fsanitize=address,undefined if g++ can link and run such a program here, else nothing"""
    src, exe = tmp / "probe.cpp", tmp / "probe"
    src.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    ok = subprocess.run(["g++"] + flags + ["-o", str(exe), str(src)], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode == 0
    return flags if ok and subprocess.run([str(exe)]).returncode == 0 else []


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ma_collapse")
    flags = sanitizer_flags(tmp)
    print("ma_collapse_driver: sanitizers", "on" if flags else "not available: compiled without")
    exe = tmp / "ma_collapse_driver"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-g"] + flags + ["-o", str(exe), os.path.join(ROOT, "tests", "ma_collapse_driver.cpp")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()
    return str(exe)


@pytest.mark.parametrize("name", cc.CASES)
def test_host_build_of_the_kernels_body_agrees(driver, name, tmp_path):
    m = cc.case(name)
    start, end, rc, score, mate = ddref.device_arrays(m.rec)
    vote = ref.not_dropped(m)
    path = str(tmp_path / "in.txt")
    with open(path, "w") as f:
        f.write("%d %d\n" % (m.L, len(m.rec)))
        for i, r in enumerate(m.rec):
            n = r["end"] - r["start"] + 1
            f.write("%d %d %d %d %d %d %s\n" % (start[i], end[i], rc[i], score[i], mate[i], vote[i], r["seq"][:n] if n else "."))
    got = subprocess.run([driver, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert got.returncode == 0, got.stderr.decode("latin1")[-2000:]
    lines = got.stdout.decode().split("\n")
    assert len(lines) == 4 * len(cc.TOLERANCES) + 1
    for k, t in enumerate(cc.TOLERANCES):
        out, _keep, members, hist, n_collapsed, n_changed, _totals = want(name, t)
        assert [int(x) for x in lines[4 * k].split()] == [t, n_collapsed, n_changed], (name, t)
        seq = "".join(r["seq"][:r["end"] - r["start"] + 1] for r in out)
        assert lines[4 * k + 1] == (seq or "."), (name, t)
        assert np.array_equal(np.array(lines[4 * k + 2].split(), np.int32), members), (name, t)
        assert np.array_equal(np.array(lines[4 * k + 3].split(), np.int64).reshape(2, 6, 6), hist), (name, t)


def test_collapse_symbols_declared_exported_and_bound():
    import mia_amd
    hdr = open(os.path.join(ROOT, "include", "mia_hip.h")).read()
    declared = set(re.findall(r"\b(mia_hip_[a-z_0-9]+)\s*\(", hdr))
    lib = mia_amd.lib()
    for sym in ("mia_hip_ma_collapse", "mia_hip_get_ma_collapse"):
        assert sym in declared, sym
        assert sym in mia_amd.exported_symbols(), sym
        assert hasattr(lib, sym), sym
    assert hasattr(mia_amd.MiaHip, "ma_collapse")
    src = open(os.path.join(ROOT, "mapping-iterative-assembler_amd", "csrc", "mia_hip.hip")).read()
    table = re.search(r"STAGE_NAMES_MORE\[STG_ALL - STG_COUNT\] = \{(.*?)\};", src, re.S).group(1)
    assert re.findall(r'"([a-z_0-9]+)"', table) == mia_amd.MiaHip.STAGES_ALWAYS_TIMED == ["k_ma_collapse_plan", "k_ma_collapse_count", "k_ma_collapse_decide"]
    assert not set(mia_amd.MiaHip.STAGES_ALWAYS_TIMED) & set(mia_amd.MiaHip.STAGES)
    body = open(os.path.join(ROOT, "mapping-iterative-assembler_amd", "csrc", "ma_collapse_body.h")).read()
    assert int(re.search(r"MA_COL_K = (\d+);", body).group(1)) == cc.K
    for f in ("csrc/ma_collapse_body.h", "csrc/mia_ma_collapse_kernels.h", "host/maln_collapse.h"):
        assert os.path.exists(os.path.join(ROOT, "mapping-iterative-assembler_amd", f))


# ---- against the compiled reference: tests/golden/ma_collapse, made by tools/make_ma_collapse_goldens.py ----------------------------
def _gold():
    with gzip.open(os.path.join(ROOT, "tests", "golden", "ma_collapse", "outputs.json.gz")) as f:
        return json.load(f)


def _same(text, recorded, what):
    text = text.encode("latin1")
    if isinstance(recorded, dict):
        assert (len(text), hashlib.sha256(text).hexdigest()) == (recorded["bytes"], recorded["sha256"]), what
    else:
        assert text == recorded.encode("latin1"), what


@pytest.mark.parametrize("t", (0, 2))
@pytest.mark.parametrize("name", cc.CASES)
def test_the_collapsed_file_reads_as_the_reference_read_it(name, t):
    """the reference's `ma -f 41 -c 1` and `ma -f 5` on the file the restatement collapsed, against maln_synth's own restatement of
    those two formats on the same records: the rewrite leaves a file the reference reads as intended"""
    gold = _gold()["cases"][name][str(t)]
    m = cc.case(name)
    new, _members, hist = ref.collapse(m, t, ref.not_dropped(m))
    assert gold["hist"] == [int(x) for x in hist.reshape(-1)]
    r = ms.restate(new)
    for tag, key in (("f41c1", "f41c1"), ("f5", "f5c1")):
        _same(r.output(key), gold[tag], (name, t, tag))


def test_the_references_own_runs_show_the_paths_the_goldens_rest_on():
    """tests/golden/ma_dedup/reads_a, reads_b at tolerance 0: 1 and 8 columns change to another base, own stays on 12 and 19 ties, no '-'
    wins and no N appears; the recorded counts are the restatement's"""
    gold = _gold()["sets"]
    seen = {}
    for name in ("reads_a", "reads_b"):
        with gzip.open(os.path.join(ROOT, "tests", "golden", "ma_dedup", name + ".maln.1.gz"), "rt", encoding="latin1") as f:
            m = ms.parse_maln(f.read().split("\n", 1)[1])
        for t in (0, 2):
            hist = ref.collapse_records(m, t, ref.not_dropped(m))[3]
            assert gold[name][str(t)]["hist"] == [int(x) for x in hist.reshape(-1)]
            if t == 0:
                seen[name] = hist.sum(axis=(0, 1))[3:].tolist()
        _keep, _rep, clusters, _totals = ref.clusters_of(m.rec, m.L, 0)
        assert sum(1 for best, mols in clusters if len(mols) >= 2 for R in best[5] if m.rec[R]["seg"] in "fb") == 8
    assert seen == {"reads_a": [1, 0, 0], "reads_b": [8, 0, 0]}
