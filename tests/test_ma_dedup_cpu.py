"""The duplicate filter (ma_hip -u, -t) without a GPU.  tests/ma_dedup_ref.py restates the rule of DESIGN.md ("Duplicate
filter": the reference's sort_fsdb + set_uniq_in_fsdb with just_outer_coords and a tolerance) as a sort and a serial walk; here it is
held to a table written out by hand, to a plain group-by at tolerance 0 and to itself under a permutation of the records.  The code
the kernels run per lane (csrc/ma_dedup_body.h) is compiled for the host into tests/ma_dedup_driver.cpp, with
-fsanitize=address,undefined where g++ has that runtime, run as a program of its own: its staged form (radix sort, runs, next,
doubling, scan) must agree with its own serial walk and with the restatement for every case and every tolerance."""
import os
import re
import subprocess

import numpy as np
import pytest

import ma_dedup_ref as ref
import maln_dedup_cases as dc
from conftest import ROOT

CPU_CASES = tuple(n for n in dc.CASES)
_want = {}


def want(name, t):
    if (name, t) not in _want:
        m = dc.case(name)
        _want[name, t] = ref.dedup(m.rec, m.L, t)
    return _want[name, t]


def test_the_hand_table():
    m = dc.case("hand")
    ids = [r["id"] for r in m.rec]
    assert ids == ["h0", "h1", "h2", "r_low", "r_a", "r_b", "q0", "q1", "q2", "q3", "h0_again"]
    #                    h0  h1 h2 r_low r_a r_b q0 q1 q2 q3 h0_again
    table = {0: ([0, 1, 1, 0, 1, 0, 1, 1, 1, 1, 1], [10, 1, 2, 4, 4, 4, 6, 7, 8, 9, 10], 8, {(0, 1): 6, (0, 2): 1, (1, 3): 1}),
             # (0,100) (0,90) (1,100) are three anchors although the third lies within 1 of the first; q1 joins q0, q3 joins q2;
             # q1 scores higher than q0 and is still not the representative
             1: ([0, 1, 1, 0, 1, 0, 1, 0, 1, 0, 1], [10, 1, 2, 4, 4, 4, 6, 6, 8, 8, 10], 6, {(0, 1): 2, (0, 2): 3, (1, 3): 1}),
             # starts 200, 201, 202 are one cluster and 203 is the next: the comparison is with the anchor 200, not with 202
             2: ([0, 1, 1, 0, 1, 0, 1, 0, 0, 1, 1], [10, 1, 2, 4, 4, 4, 6, 6, 6, 9, 10], 6, {(0, 1): 3, (0, 2): 1, (0, 3): 1, (1, 3): 1})}
    for t, (keep, rep, clusters, sizes) in table.items():
        got = ref.dedup(m.rec, m.L, t)
        assert got[0].tolist() == keep and got[1].tolist() == rep, t
        assert got[3:] == (11, clusters, 0), t
        hist = np.zeros((2, ref.SIZES), np.int64)
        for (rc, size), k in sizes.items():
            hist[rc, size] = k
        assert np.array_equal(got[2], hist), t


def test_orphans_and_pairs_of_the_wrap_case():
    m = dc.case("wrap")
    mate = ref.pair_halves(m.rec)
    by_id = {}
    for i, r in enumerate(m.rec):
        by_id.setdefault(r["id"], []).append(i)
    for rid in ("no_mate_f", "twice_f", "twice_b", "strands_f", "strands_b", "no_suffix"):
        assert all(mate[i] == -2 for i in by_id[rid]), rid
    for stem in ("w1f", "w2f", "w3f", "w1r", "w2r", "w3r"):
        f, b = by_id[stem + "_f"][0], by_id[stem + "_b"][0]
        assert mate[f] == b and mate[b] == f
    keep, rep, _hist, n_mol, _n_clu, orphans = ref.dedup(m.rec, m.L, 0)
    assert orphans == 7 and n_mol == len(m.rec) - 7 - 6
    for t in "fr":
        f1, b1, f2, b2 = (by_id[k % t][0] for k in ("w1%s_f", "w1%s_b", "w2%s_f", "w2%s_b"))
        assert keep[[f1, b1, f2, b2]].tolist() == [0, 0, 1, 1]            # the pair with the better front score, both halves
        assert rep[[f1, b1, f2, b2]].tolist() == [min(f2, b2)] * 4        # its index: the back half comes first in the file
        assert keep[by_id["whole" + t][0]] == 1 and keep[by_id["back_alone" + t][0]] == 1
    assert all(keep[i] == 1 and rep[i] == i for rid in ("no_mate_f", "twice_f", "no_suffix") for i in by_id[rid])
    # with t = 7 the pair that ends 6 columns later joins the cluster of the one that sorts first: on the forward strand e descending
    keep7 = ref.dedup(m.rec, m.L, 7)[0]
    assert keep7[by_id["w3f_f"][0]] == 1 and keep7[by_id["w2f_f"][0]] == 0


@pytest.mark.parametrize("name", CPU_CASES)
def test_tolerance_0_is_a_group_by(name):
    m = dc.case(name)
    keep, rep, hist, n_mol, n_clu, orphans = want(name, 0)
    groups = ref.group_by(m.rec, m.L)
    assert n_clu == len(groups) and n_mol == sum(len(g) for g in groups.values())
    sizes = np.zeros((2, ref.SIZES), np.int64)
    kept = np.zeros(len(m.rec), np.uint8)
    for (rc, _a, _e), mols in groups.items():
        sizes[rc, min(len(mols), ref.SIZES - 1)] += 1
        best = max(mols, key=lambda x: (x[3], -x[4]))
        for x in mols:
            for r in x[5]:
                assert rep[r] == best[4]
        for r in best[5]:
            kept[r] = 1
    kept[ref.pair_halves(m.rec) == -2] = 1
    assert np.array_equal(keep, kept) and np.array_equal(hist, sizes)
    assert orphans == int((ref.pair_halves(m.rec) == -2).sum())


@pytest.mark.parametrize("name", ("hand", "e_ladder", "wrap", "stairs_rev", "runs_edge"))
@pytest.mark.parametrize("t", (0, 2))
def test_a_permutation_of_the_records_permutes_the_result(name, t):
    """where scores do not tie: the scores are made distinct first (the index breaks ties, and it moves with the permutation)"""
    m = dc.case(name)
    recs = [dict(r, score=r["score"] * 100000 + i) for i, r in enumerate(m.rec)]
    perm = dc.ms.Rng(77).permutation(len(recs)).tolist()
    moved = [recs[p] for p in perm]                                  # moved[j] = recs[perm[j]]
    a, b = ref.dedup(recs, m.L, t), ref.dedup(moved, m.L, t)
    assert np.array_equal(b[0], a[0][perm])
    pos = np.argsort(perm)                                           # where record i went
    for j, p in enumerate(perm):
        if ref.pair_halves(recs)[p] != -1:
            continue                                                 # (a pair's index is the lower of two numbers: it need not move with them)
        rep_old = a[1][p]
        if ref.pair_halves(recs)[rep_old] == -1:
            assert b[1][j] == pos[rep_old]
    assert np.array_equal(a[2], b[2]) and a[3:] == b[3:]


def test_gaps_fall_only_where_no_kept_record_has_the_insert():
    m = dc.case("ins_only_in_dups")
    keep = want("ins_only_in_dups", 0)[0]
    assert [r["id"] for r, k in zip(m.rec, keep) if k] == ["best", "alone", "alone_rev"]
    before, after = m.gaps, ref.new_gaps(m, keep)
    assert (before[30], before[40], before[50], before[105], before[107]) == (2, 3, 2, 2, 1)
    assert (after[30], after[40], after[50], after[105], after[107]) == (0, 1, 0, 2, 1)
    changed = np.nonzero(before != after)[0].tolist()
    assert changed == [30, 40, 50]


def test_of_two_pairs_for_one_position_the_later_counts():
    m = dc.case("ins_repeat")
    keep = ref.dedup(m.rec, m.L, 0)[0]
    assert keep.tolist() == [1, 0]
    before, after = m.gaps, ref.new_gaps(m, keep)
    assert (before[25], before[29], before[50]) == (3, 2, 4) and (after[25], after[29], after[50]) == (1, 2, 0)
    assert np.nonzero(before != after)[0].tolist() == [25, 50]


def sanitizer_flags(tmp):
    """-fsanitize=address,undefined if g++ can link and run such a program here, else nothing"""
    src, exe = tmp / "probe.cpp", tmp / "probe"
    src.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    ok = subprocess.run(["g++"] + flags + ["-o", str(exe), str(src)], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode == 0
    return flags if ok and subprocess.run([str(exe)]).returncode == 0 else []


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ma_dedup")
    flags = sanitizer_flags(tmp)
    print("ma_dedup_driver: sanitizers", "on" if flags else "not available: compiled without")
    exe = tmp / "ma_dedup_driver"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-g"] + flags + ["-o", str(exe), os.path.join(ROOT, "tests", "ma_dedup_driver.cpp")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()
    return str(exe)


@pytest.mark.parametrize("name", CPU_CASES + dc.LIBRARY_ONLY)
def test_host_build_of_the_kernels_body_agrees(driver, name, tmp_path):
    m = dc.case(name)
    start, end, rc, score, mate = ref.device_arrays(m.rec)
    path = str(tmp_path / "in.txt")
    with open(path, "w") as f:
        f.write("%d %d\n" % (m.L, len(m.rec)))
        f.write("".join("%d %d %d %d %d\n" % row for row in zip(start.tolist(), end.tolist(), rc.tolist(), score.tolist(), mate.tolist())))
    got = subprocess.run([driver, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert got.returncode == 0, got.stderr.decode("latin1")[-2000:]
    lines = got.stdout.decode().split("\n")
    assert len(lines) == 4 * len(dc.TOLERANCES) + 1
    for k, t in enumerate(dc.TOLERANCES):
        keep, rep, hist, n_mol, n_clu, orphans = want(name, t)
        assert [int(x) for x in lines[4 * k].split()] == [t, n_mol, n_clu, orphans], (name, t)
        assert np.array_equal(np.array(lines[4 * k + 1].split(), np.uint8), keep), (name, t)
        assert np.array_equal(np.array(lines[4 * k + 2].split(), np.int64), rep), (name, t)
        pairs = [int(x) for x in lines[4 * k + 3].split()]
        sparse = np.zeros(2 * ref.SIZES, np.int64)
        sparse[pairs[0::2]] = pairs[1::2]
        assert np.array_equal(sparse.reshape(2, ref.SIZES), hist), (name, t)


def test_dedup_symbols_declared_exported_and_bound():
    import mia_amd
    hdr = open(os.path.join(ROOT, "include", "mia_hip.h")).read()
    declared = set(re.findall(r"\b(mia_hip_[a-z_0-9]+)\s*\(", hdr))
    lib = mia_amd.lib()
    for sym in ("mia_hip_ma_dedup", "mia_hip_get_ma_dedup"):
        assert sym in declared, sym
        assert sym in mia_amd.exported_symbols(), sym
        assert hasattr(lib, sym), sym
    assert hasattr(mia_amd.MiaHip, "ma_dedup")
    mine = [s for s in mia_amd.MiaHip.STAGES if s.startswith("k_ma_dedup")]
    assert mine == ["k_ma_dedup_keys", "k_ma_dedup_sort", "k_ma_dedup_runs", "k_ma_dedup_next", "k_ma_dedup_anchors", "k_ma_dedup_clusters"]
    at = mia_amd.MiaHip.STAGES.index("k_ma_dedup_keys")
    assert mia_amd.MiaHip.STAGES[at - 1] == "k_ma_profile" and mia_amd.MiaHip.STAGES[at + 6] == "k_ma_tally"      # in front of the record upload
    src = open(os.path.join(ROOT, "mapping-iterative-assembler_amd", "csrc", "mia_hip.hip")).read()
    table = re.search(r"STAGE_NAMES\[STG_COUNT\] = \{(.*?)\};", src, re.S).group(1)
    assert re.findall(r'"([a-z_0-9]+)"', table) == mia_amd.MiaHip.STAGES
    for f in ("ma_dedup_body.h", "mia_ma_dedup_kernels.h"):
        assert os.path.exists(os.path.join(ROOT, "mapping-iterative-assembler_amd", "csrc", f))


# ---- against the compiled reference: tests/golden/ma_dedup, made by tools/make_ma_dedup_goldens.py -----------------------------------
GOLD = os.path.join(ROOT, "tests", "golden", "ma_dedup")


def _five(rows):
    return sorted((rc, start, end, seg, score) for _id, rc, start, end, seg, score, _dr, _ins in rows)


def _gold(name):
    import gzip
    import json
    with gzip.open(os.path.join(GOLD, name)) as f:
        return json.load(f)


@pytest.mark.parametrize("plain,u", (("plain", "u"), ("plain_cut", "u_cut")))
@pytest.mark.parametrize("name", dc.READ_SETS)
def test_tolerance_0_on_the_references_run_gives_its_own_u_run(name, plain, u):
    """runs.json.gz: the reference's `mia -c -n -H 1` and `mia -c -n -H 1 -u` on one read set, and the same two with the default score
    cut.  The restatement, applied to the records of the run without -u, leaves the multiset of (RC, START, END, SEG, SCORE) and the
    GAPS line of the run with it.  No IDs are compared, so ties cannot matter."""
    import maln_synth as ms
    runs = _gold("runs.json.gz")[name]
    m = ms.Maln()
    m.rec = [dict(id=i, rc=rc, start=s, end=e, seg=seg, score=sc, ins=[tuple(x) for x in ins]) for i, rc, s, e, seg, sc, _dr, ins in runs[plain]["records"]]
    m.gaps = np.array(runs[plain]["gaps"], np.int32)
    m.L = len(m.gaps)
    assert sum(1 for r in m.rec if r["seg"] == "f") >= 20 and {r["rc"] for r in m.rec} == {0, 1}
    keep = ref.dedup(m.rec, m.L, 0)[0]
    assert _five(row for row, k in zip(runs[plain]["records"], keep) if k) == _five(runs[u]["records"])
    assert ref.new_gaps(m, keep).tolist() == runs[u]["gaps"]
    if name == "reads_b":
        assert (np.array(runs[u]["gaps"]) < m.gaps).any()                   # GAPS falls somewhere


@pytest.mark.parametrize("t", (0, 2))
@pytest.mark.parametrize("name", CPU_CASES)
def test_the_reduced_file_reads_as_the_reference_read_it(name, t):
    """outputs.json.gz, "cases": the reference's `ma -f 41 -c 1` and `ma -f 5` on the file the restatement has reduced, against
    maln_synth's own restatement of those two formats on the same reduced records (GAPS recomputed): the removal leaves a file the
    reference reads"""
    import hashlib
    import maln_synth as ms
    gold = _gold("outputs.json.gz")["cases"][name][str(t)]
    m = dc.case(name)
    r = ms.restate(ref.reduce(m, want(name, t)[0]))
    for tag, key in (("f41c1", "f41c1"), ("f5", "f5c1")):
        text = r.output(key).encode("latin1")
        if isinstance(gold[tag], dict):
            assert (len(text), hashlib.sha256(text).hexdigest()) == (gold[tag]["bytes"], gold[tag]["sha256"]), (name, t, tag)
        else:
            assert text == gold[tag].encode("latin1"), (name, t, tag)
