"""The damage score (ma_hip -L, -K, -S, -f 97) without a GPU.  tests/ma_pmd_ref.py restates the rule of DESIGN.md ("Damage score") as a
loop over records and columns and a dictionary of molecules; here it is held to a table written out by hand and to itself under a
permutation of the records, and the library's model table (mia_hip_ma_pmd_table: host arithmetic, no device) to the restatement's.
The code the kernels run per lane (csrc/ma_pmd_body.h) is compiled for the host into tests/ma_pmd_driver.cpp, with
-fsanitize=address,undefined where g++ has that runtime, run as a program of its own: its stretches must agree with its own walk
record by record and with the restatement for every case, use mask, weight table and threshold."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import ma_dedup_ref
import ma_pmd_ref as ref
import maln_pmd_cases as pc
import maln_synth as ms
from conftest import ROOT
from test_ma_damage_cpu import sanitizer_flags

A, C, G, T = 0, 1, 2, 3
OTHER_MODEL = (0.2, 0.02, 0.001, 0.0005)
_ev = {}


def events(name):
    if name not in _ev:
        _ev[name] = ref.events(pc.case(name)[0])
    return _ev[name]


def test_the_hand_table():
    m, masks = pc.case("signs")
    w = pc.hand_table()
    assert [r["id"] for r in m.rec] == pc.SIGNS_IDS
    mate = ma_dedup_ref.pair_halves(m.rec)
    assert mate.tolist() == [-1, -1, -1, -1, -1, -1, 7, 6, 9, 8, 11, 10, -1, -1, -1, -2, -1, -1]
    #            neg1 neg32768 neg32769 zero five four up_f up_b down_f down_b low_b low_f     top   bottom   floor0 orph_f rev drop
    want_rec = [-1, -32768, -32769, 0, 5, 4, 6, -1, 6, -2, 3, -32768, 2097152, -688128, -655360, 3, 2, 3]
    want_mol = [-1, -32768, -32769, 0, 5, 4, 5, 5, 4, 4, -32765, -32765, 2097152, -688128, -655360, 3, 2, 3]
    rec, mol, keep, hist, n_mol, n_kept, orphans = ref.score(m, w, pc.SIGNS_THRESHOLD)
    assert rec.tolist() == want_rec and mol.tolist() == want_mol
    assert "".join(str(k) for k in keep) == "000010110000100000" and (n_mol, n_kept, orphans) == (15, 4, 1)
    want = np.zeros((2, 64), np.int64)
    want[0, 19], want[0, 18], want[0, 20], want[0, 63], want[0, 0], want[1, 20] = 3, 1, 7, 1, 2, 1
    assert np.array_equal(hist, want)
    # the bins: a floor division also below zero, half a nat each, clamped at both ends
    assert [ref.bin_of(S) for S in (-1, -32768, -32769, 0, 32767, 32768, -655360, -655361, -10 ** 12, 1409023, 1409024, 10 ** 12)] == \
        [19, 19, 18, 20, 20, 21, 0, 0, 0, 62, 63, 63]
    # thresholds on either side
    assert "".join(str(k) for k in ref.score(m, w, 0)[2]) == "000111111100100111"
    assert "".join(str(k) for k in ref.score(m, w, 6)[2]) == "000000000000100000"
    assert ref.score(m, w, -10 ** 9)[5] == 18 and ref.score(m, w, 10 ** 9)[5] == 0
    # one half switched off: the molecule's sum changes sides, and it still counts
    got = ref.score(m, w, pc.SIGNS_THRESHOLD, masks[0])
    assert got[0][7] == 0 and got[1][6] == got[1][7] == 6 and got[2][6] == got[2][7] == 1 and got[4] == 15
    got = ref.score(m, w, pc.SIGNS_THRESHOLD, masks[1])
    assert got[0][8] == 0 and got[1][8] == got[1][9] == -2 and got[2][8] == got[2][9] == 0 and got[4] == 15 and got[3][0, 19] == 4 and got[3][0, 20] == 6
    # both halves off: S = 0 >= threshold 0 keeps it, but it counts nowhere
    got = ref.score(m, w, 0, masks[2])
    assert got[1][10] == got[1][11] == 0 and got[2][10] == got[2][11] == 1 and got[4] == 14 and got[3][0, 19] == 2
    # the dropped record left out
    use = np.array([0 if r["dr"] else 1 for r in m.rec], np.uint8)
    assert ref.score(m, w, 0, use)[4] == 14
    assert threshold_pairs() == [(3, 196608), (0, 0), (-0.5, -32768), (2.5e-6, 0), (8e-6, 1)]


def threshold_pairs():
    return [(x, ref.threshold_of(x)) for x in (3, 0, -0.5, 2.5e-6, 8e-6)]


def test_table_text_from_a_hist_written_by_hand():
    hist = np.zeros((2, 64), np.int64)
    hist[0, 0], hist[0, 20], hist[1, 20], hist[1, 26], hist[0, 63] = 2, 5, 1, 3, 4
    text = ref.table_of(hist, 1, 17, False).split("\n")
    assert text[0] == "# ma_hip damage scores: 15 molecules, 1 orphan halves, 17 records, library ds, p 0.3 c0 0.01 pi 0.001 eps 0.000333333"
    assert text[1] == "# from\t+\t-\tall\tfrom+\tfrom-\tfrom_all"
    assert text[2] == "-inf\t2\t0\t2\t11\t4\t15"
    assert text[3] == "-9.5\t0\t0\t0\t9\t4\t13"
    assert text[22] == "0.0\t5\t1\t6\t9\t4\t13"
    assert text[23] == "0.5\t0\t0\t0\t4\t3\t7"
    assert text[28] == "3.0\t0\t3\t3\t4\t3\t7"
    assert text[29] == "3.5\t0\t0\t0\t4\t0\t4"
    assert text[65] == "21.5\t4\t0\t4\t4\t0\t4"
    assert len(text) == 67 and text[66] == ""
    assert ref.table_of(np.zeros((2, 64), np.int64), 0, 0, True, OTHER_MODEL).split("\n")[0].endswith("0 records, library ss, p 0.2 c0 0.02 pi 0.001 eps 0.0005")
    empty = ref.table(pc.case("empty")[0], ref.model_table())
    assert [line.split("\t")[1:] for line in empty.split("\n")[2:66]] == [["0"] * 6] * 64


def test_the_models_table():
    ds, ss = ref.model_table(), ref.model_table(ss=True)
    assert int(np.abs(ds).max()) == 357304 == int(ds[0, C, T]) == int(ds[30, G, A]) == int(ss[30, C, T])
    # MIDDLE by hand: D = c0; 1 - L(0) = pi + eps - 2 pi eps, 1 - L(D) = (1 - D)(1 - L(0)) + D (1 - (1 - pi) eps)
    pi, eps = 0.001, 0.001 / 3
    miss0 = pi + eps - 2 * pi * eps
    miss = 0.99 * miss0 + 0.01 * (1 - (1 - pi) * eps)
    assert abs(int(ds[15, C, T]) - math.log(miss / miss0) * 65536) <= 1 and abs(int(ds[15, C, C]) - math.log((1 - miss) / (1 - miss0)) * 65536) <= 1
    assert np.array_equal(ds[15, G], np.array([ds[15, C, T], 0, ds[15, C, C], 0, 0]))
    for w in (ds, ss):
        zero = np.ones((31, 5, 5), bool)
        zero[:, C, C] = zero[:, C, T] = False
        if w is ds:
            zero[:, G, G] = zero[:, G, A] = False
        assert not w[zero].any() and (w[:, C, T] > 0).all() and (w[:, C, C] < 0).all()
    # the 5' weights fall with the position, MIDDLE and the 3' half of a double-stranded library's C rows are the background's
    assert (np.diff(ds[:16, C, T]) < 0).all() and (ds[15:, C, T] == ds[15, C, T]).all() and (ds[:16, G, A] == ds[15, G, A]).all()
    assert np.array_equal(ds[:, G, A], ds[::-1, C, T]) and np.array_equal(ss[:, C, T], np.maximum(ds[:, C, T], ds[::-1, C, T]))


def test_the_librarys_model_table_is_the_restatements():
    import mia_amd
    for params in (ref.DEFAULTS, OTHER_MODEL, (0.9, 0.0, 0.5, 0.5), (1e-3, 0.5, 1e-9, 1e-9)):
        for ss in (False, True):
            got, want = mia_amd.ma_pmd_table(*params, single_stranded=ss), ref.model_table(*params, ss=ss)
            assert got.dtype == np.int32 and got.shape == (31, 5, 5)
            assert np.abs(got.astype(np.int64) - want).max() <= 1, (params, ss)            # (two implementations of log)
            assert not got[want == 0].any(), (params, ss)
    assert np.array_equal(mia_amd.ma_pmd_table(), mia_amd.ma_pmd_table(*ref.DEFAULTS))
    nan, inf = float("nan"), float("inf")
    for bad in ((0.0, 0.01, 0.001, 0.001), (1.0, 0.01, 0.001, 0.001), (0.3, -0.01, 0.001, 0.001), (0.3, 1.0, 0.001, 0.001), (0.3, 0.01, 0.0, 0.001),
                (0.3, 0.01, 1.0, 0.001), (0.3, 0.01, 0.001, 0.0), (0.3, 0.01, 0.001, 1.0), (0.3, 0.75, 0.001, 0.001), (0.5, 0.6, 0.001, 0.001),
                (nan, 0.01, 0.001, 0.001), (0.3, nan, 0.001, 0.001), (0.3, 0.01, inf, 0.001), (0.3, 0.01, 0.001, -inf)):
        assert ref.model_table(*bad) is None and ref.model_table(*bad, ss=True) is None, bad
        for ss in (False, True):
            with pytest.raises(ValueError):
                mia_amd.ma_pmd_table(*bad, single_stranded=ss)
    assert mia_amd.lib().mia_hip_ma_pmd_table(0.3, 0.01, 0.001, 0.001, 0, None) == -2         # MIA_HIP_ERR_ARG
    assert mia_amd.ma_pmd_table(0.3, 0.699, 0.001, 0.001) is not None


def test_cases_hold_what_they_promise():
    assert set(pc.dc.CASES) < set(pc.CASES)
    m, _ = pc.case("edges")                                  # (its own assertions hold every begin and end)
    assert {len(r["seq"]) for r in m.rec} >= set(pc.EDGE_LENS)
    m, _ = pc.case("span3")
    assert [len(r["seq"]) for r in m.rec] == [100, 9000, 40]
    m, _ = pc.case("big")
    for tag, w in pc.own_tables("big"):
        rec = ref.record_scores(m, w, ev=events("big"))
        assert abs(int(rec[0])) > 2 ** 32 and (rec[0] > 0) == (tag == "plus")
    m, _ = pc.case("signs")
    rec = ref.record_scores(m, pc.hand_table(), ev=events("signs"))
    mate = ma_dedup_ref.pair_halves(m.rec)
    opposite = [r for r in range(len(m.rec)) if mate[r] > r and rec[r] * rec[mate[r]] < 0]
    assert len(opposite) == 3
    sums = sorted(int(rec[r] + rec[mate[r]]) for r in opposite)
    assert sums[1] < pc.SIGNS_THRESHOLD <= sums[2]


@pytest.mark.parametrize("name", ("signs", "wrap", "mixed", "offsets"))
def test_a_permutation_of_the_records_permutes_the_result(name):
    m, _ = pc.case(name)
    perm = ms.Rng(79).permutation(len(m.rec)).tolist()
    moved = ms.Maln()
    moved.L, moved.ref_seq, moved.gaps = m.L, m.ref_seq, m.gaps
    moved.rec = [m.rec[p] for p in perm]
    for tag, w in pc.tables(name, ref.model_table(), ref.model_table(ss=True)):
        a = ref.score(m, w, 3 * 65536, ev=events(name))
        b = ref.score(moved, w, 3 * 65536, ev=[events(name)[p] for p in perm])
        for k in range(3):
            assert np.array_equal(b[k], a[k][perm]), (name, tag, k)
        assert a[4:] == b[4:] and np.array_equal(a[3], b[3]), (name, tag)
    if name == "signs":
        other, _ = pc.case("signs_permuted")
        assert sorted(r["id"] for r in other.rec) == sorted(pc.SIGNS_IDS) and [r["id"] for r in other.rec] != pc.SIGNS_IDS
        a, b = ref.score(m, pc.hand_table(), pc.SIGNS_THRESHOLD), ref.score(other, pc.hand_table(), pc.SIGNS_THRESHOLD)
        assert np.array_equal(a[3], b[3]) and a[4:] == b[4:]
        assert {r["id"]: int(b[1][k]) for k, r in enumerate(other.rec)} == {r["id"]: int(a[1][k]) for k, r in enumerate(m.rec)}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ma_pmd")
    flags = sanitizer_flags(tmp)
    print("ma_pmd_driver: sanitizers", "on" if flags else "not available: compiled without")
    exe = tmp / "ma_pmd_driver"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-g"] + flags + ["-o", str(exe), os.path.join(ROOT, "tests", "ma_pmd_driver.cpp")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()
    return str(exe)


@pytest.mark.parametrize("name", pc.CASES)
def test_host_build_of_the_kernels_body_agrees(driver, name, tmp_path):
    m, _ = pc.case(name)
    f = ms.flatten(m)
    mate = ma_dedup_ref.pair_halves(m.rec)
    tabs = pc.tables(name, ref.model_table(), ref.model_table(ss=True))
    for which, use in enumerate(pc.uses(name)):
        plans = []
        for tag, w in tabs:
            rec = ref.record_scores(m, w, use, events(name))
            plans.append((tag, w, rec, pc.thresholds(name, ref.score(m, w, 0, use, mate, rec)[1])))
        path = str(tmp_path / ("in%d.txt" % which))
        with open(path, "w", encoding="latin1") as out:
            out.write("%d %d %d\n%s\n>%s\n>%s\n" % (m.L, len(m.rec), f["col_off"][-1], m.ref_seq, f["seq"].tobytes().decode("latin1"), f["smp"].tobytes().decode("latin1")))
            for r in range(len(m.rec)):
                out.write("%d %d %d %d %d\n" % (f["start"][r], f["revcom"][r], 1 if use is None else use[r], mate[r], f["col_off"][r + 1]))
            out.write("%d %d\n" % (len(plans), len(plans[0][3])))
            for _tag, w, _rec, thr in plans:
                out.write(" ".join(str(int(x)) for x in w.ravel()) + "\n" + " ".join(str(t) for t in thr) + "\n")
        got = subprocess.run([driver, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert got.returncode == 0, got.stderr.decode("latin1")[-2000:]
        lines = got.stdout.decode().split("\n")
        assert len(lines) == sum(1 + 4 * len(p[3]) for p in plans) + 1
        at = 0
        for tag, w, rec, thr in plans:
            assert np.array_equal(np.array(lines[at].split()[1:], np.int64), rec), (name, which, tag)
            at += 1
            for threshold in thr:
                _rec, mol, keep, hist, n_mol, n_kept, orphans = ref.score(m, w, threshold, use, mate, rec)
                assert [int(x) for x in lines[at].split()] == [threshold, n_mol, n_kept, orphans], (name, which, tag, threshold)
                assert lines[at + 1] == ("".join(str(x) for x in keep) or "-"), (name, which, tag, threshold)
                assert np.array_equal(np.array(lines[at + 2].split()[1:], np.int64), mol), (name, which, tag, threshold)
                pairs = [int(x) for x in lines[at + 3].split()[1:]]
                sparse = np.zeros(128, np.int64)
                sparse[pairs[0::2]] = pairs[1::2]
                assert np.array_equal(sparse.reshape(2, 64), hist), (name, which, tag, threshold)
                at += 4


def test_score_symbols_declared_exported_and_bound():
    import mia_amd
    hdr = open(os.path.join(ROOT, "include", "mia_hip.h")).read()
    declared = set(re.findall(r"\b(mia_hip_[a-z_0-9]+)\s*\(", hdr))
    lib = mia_amd.lib()
    for sym in ("mia_hip_ma_pmd_table", "mia_hip_ma_score", "mia_hip_get_ma_score"):
        assert sym in declared, sym
        assert sym in mia_amd.exported_symbols(), sym
        assert hasattr(lib, sym), sym
    assert hasattr(mia_amd.MiaHip, "ma_score") and hasattr(mia_amd, "ma_pmd_table")
    stages = mia_amd.MiaHip.STAGES
    at = stages.index("k_ma_score_cols")
    assert stages[at:at + 2] == ["k_ma_score_cols", "k_ma_score_molecules"]
    src = open(os.path.join(ROOT, "mapping-iterative-assembler_amd", "csrc", "mia_hip.hip")).read()
    table = re.search(r"STAGE_NAMES\[STG_COUNT\] = \{(.*?)\};", src, re.S).group(1)
    assert re.findall(r'"([a-z_0-9]+)"', table) == stages
    assert len(stages) <= 32                                 # a bit per stage in mia_hip_set_stage_mask
    for f in ("ma_pmd_body.h", "mia_ma_pmd_kernels.h"):
        assert os.path.exists(os.path.join(ROOT, "mapping-iterative-assembler_amd", "csrc", f))
