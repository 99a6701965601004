"""The end mask (ma_hip -E, -x, -f 96) without a GPU.  tests/ma_mask_ref.py restates the rule of DESIGN.md ("End mask") as a loop over
records and columns; here it is held to records worked out by hand, to the counts recorded beside the compiled reference's outputs
(tests/golden/ma_mask), and to the project's own restated tally: trimming commutes with tallying.  The code the kernels run per lane
(csrc/ma_mask_body.h) is compiled for the host into tests/ma_mask_driver.cpp, with -fsanitize=address,undefined where g++ has that
runtime, run as a program of its own: its stretches must agree with its own walk record by record and with the restatement for every
case and setting."""
import gzip
import json
import os
import re
import subprocess

import numpy as np
import pytest

import ma_mask_ref as ref
import maln_ace_cases as mc
import maln_mask_cases as kc
import maln_synth as ms
from conftest import ROOT

GOLD = os.path.join(ROOT, "tests", "golden", "ma_mask", "outputs.json.gz")
CODES = "ABCPPPP]^_"                       # ten columns: positions 1, 2, 3 from the 5' end, four MIDDLE, positions 3, 2, 1 from the 3' end
SEQ = "TACGTACGTA"


def one(seq, smp, rc=0, ins=(), n5=3, n3=3, x=False, ss=False, start=20):
    """the mask of a file with this one record"""
    m = mc._blank("hand", 100, ms.Rng(1), {})
    for p, s in ins:
        if 0 < p < len(seq):
            m.gaps[start + p] = len(s)
    m.rec.append({"id": "r", "desc": "d", "score": 7, "num_inputs": 2, "start": start, "end": start + len(seq) - 1, "rc": rc, "tr": 1, "dr": 0, "seg": "n",
                  "seq": seq, "smp": smp, "ins": list(ins)})
    return m, ref.mask(m, n5, n3, x, ss)


def hist_of(*entries):
    h = np.zeros((2, 2, 16), np.int64)
    for strand, end, k in entries:
        h[strand, end, k] += 1
    return h


def test_forward_and_rc_records_by_hand():
    for rc in (0, 1):
        m, got = one(SEQ, CODES, rc)
        r = got.maln.rec[0]
        assert (r["start"], r["end"], r["seq"], r["smp"]) == (23, 26, "GTAC", "PPPP")
        assert {k: r[k] for k in ("id", "desc", "score", "num_inputs", "rc", "tr", "dr", "seg")} == {k: m.rec[0][k] for k in ("id", "desc", "score", "num_inputs", "rc", "tr", "dr", "seg")}
        assert np.array_equal(got.hist, hist_of(*[(rc, e, k) for e in (0, 1) for k in (1, 2, 3)]))
        assert (got.first.tolist(), got.count.tolist(), got.start.tolist(), got.col_off.tolist()) == ([3], [4], [23], [0, 4])
        assert (got.seq, got.smp, got.emptied, got.stripped, got.pairs_dropped, got.n_kept, got.cols_kept) == (b"GTAC", b"PPPP", [0, 0], 0, 0, 1, 4)
    # one end alone; an RC record's 5' end is its last stored column
    assert one(SEQ, CODES, 0, n5=2, n3=0)[1].maln.rec[0]["seq"] == "CGTACGTA"
    assert one(SEQ, CODES, 1, n5=2, n3=0)[1].maln.rec[0]["seq"] == "TACGTACG"
    assert np.array_equal(one(SEQ, CODES, 1, n5=2, n3=0)[1].hist, hist_of((1, 0, 1), (1, 0, 2)))
    assert one(SEQ, CODES, 0, n5=0, n3=1)[1].maln.rec[0]["seq"] == "TACGTACGT"
    # MIDDLE is in no zone even at (15, 15)
    assert one(SEQ, CODES, 0, n5=15, n3=15)[1].maln.rec[0]["seq"] == "GTAC"


def test_short_reads_dashes_and_bad_codes_by_hand():
    _, got = one("TACG", "ABCD")                             # shorter than n5 + n3: codes count from the 5' end alone
    assert (got.maln.rec[0]["seq"], got.maln.rec[0]["start"], got.hist.sum()) == ("G", 23, 3)
    _, got = one("TACG", "ABCD", n5=5)
    assert (got.maln.rec, got.emptied, got.count.tolist(), got.first.tolist(), got.start.tolist(), got.n_kept) == ([], [1, 0], [0], [0], [20], 0)
    assert np.array_equal(got.hist, hist_of((0, 0, 1), (0, 0, 2), (0, 0, 3), (0, 0, 4)))
    _, got = one("TAC-TACGTA", CODES)                        # a '-' at the front boundary
    assert (got.maln.rec[0]["seq"], got.maln.rec[0]["start"], got.maln.rec[0]["end"], got.stripped) == ("TAC", 24, 26, 1)
    _, got = one("TACGTA-GTA", CODES, 1)                     # ... at the back boundary
    assert (got.maln.rec[0]["seq"], got.maln.rec[0]["start"], got.maln.rec[0]["end"], got.stripped) == ("GTA", 23, 25, 1)
    _, got = one("TAC----GTA", CODES, 1)                     # nothing but '-' between the zones
    assert (got.maln.rec, got.emptied, got.stripped, got.hist.sum()) == ([], [0, 1], 4, 6)
    _, got = one("TACGTACGTA", "ABCPAPP]^_")                 # a zone code between kept columns stays and is not counted
    assert (got.maln.rec[0]["seq"], got.maln.rec[0]["smp"], got.hist.sum()) == ("GTAC", "PAPP", 6)
    _, got = one("TA-GTACGTA", "AB~PPPP]^_")                 # a bad code is in no zone: the '-' under it is stripped, not counted
    assert (got.maln.rec[0]["seq"], got.first.tolist(), got.stripped, got.hist.sum()) == ("GTAC", [3], 1, 5)
    _, got = one("TACGTACGTA", "AB~PPPP]^_")
    assert (got.maln.rec[0]["seq"], got.maln.rec[0]["smp"], got.first.tolist()) == ("CGTAC", "~PPPP", [2])
    m, got = one("", "")                                     # a record without columns (END = START - 1)
    assert m.rec[0]["end"] == 19 and (got.maln.rec, got.emptied, got.cols_kept) == ([], [1, 0], 0)


def test_inserts_by_hand():
    ins = [(0, "AA"), (3, "A"), (4, "CC"), (6, "G"), (7, "TTT"), (9, "A")]
    m, got = one(SEQ, CODES, ins=ins)
    assert got.maln.rec[0]["ins"] == [(1, "CC"), (3, "G")]   # a < pos < b alone: not the pair at a, not the pair at b
    assert (got.pair_keep.tolist(), got.ins_pos.tolist(), got.pairs_dropped) == ([0, 0, 1, 0 + 1, 0, 0], [0, 0, 1, 3, 0, 0], 4)
    gaps = np.zeros(100, np.int32)
    gaps[24], gaps[26] = 2, 1
    assert np.array_equal(got.maln.gaps, gaps) and m.gaps[27] == 3
    _, got = one("TACG", "ABCD", n5=5, ins=[(1, "A"), (2, "C")])          # an emptied record's pairs leave with it and are not `dropped`
    assert (got.pair_keep.tolist(), got.pairs_dropped, int(got.maln.gaps.sum())) == ([0, 0], 0, 0)


def test_substitution_by_hand():
    for rc, ss, want, hist in ((0, False, "NACGTACGTN", ((0, 0, 1), (0, 1, 1))), (0, True, "NACGTACGNA", ((0, 0, 1), (0, 1, 2))),
                               (1, False, "NACGTACGTN", ((1, 1, 1), (1, 0, 1))), (1, True, "TNCGTACGTN", ((1, 1, 2), (1, 0, 1)))):
        m, got = one(SEQ, CODES, rc, ins=[(0, "A"), (5, "C")], x=True, ss=ss)
        r = got.maln.rec[0]
        assert (r["seq"], r["smp"], r["start"], r["end"], r["ins"]) == (want, CODES, 20, 29, [(0, "A"), (5, "C")]), (rc, ss)
        assert np.array_equal(got.hist, hist_of(*hist)), (rc, ss)
        assert (got.seq, got.pair_keep.tolist(), got.ins_pos.tolist(), got.n_kept, got.cols_kept) == (want.encode(), [1, 1], [0, 5], 1, 10)
        assert np.array_equal(got.maln.gaps, m.gaps)
    assert one("tacgtacgta", CODES, 0, x=True)[1].maln.rec[0]["seq"] == "NacgtacgtN"          # upper-cased for the test alone
    assert one("T-CGTACG-A", "~BCPPPP]^A", 0, x=True)[1].maln.rec[0]["seq"] == "T-CGTACG-A"      # a bad code, '-', a 5' code on an A
    assert one("TTTTTTTTTT", "PPPPPPPPPP", 0, n5=15, n3=15, x=True)[1].hist.sum() == 0


def test_report_text_from_counts_written_by_hand():
    hist = np.zeros((2, 2, 16), np.int64)
    hist[0, 0, 1], hist[1, 0, 1], hist[0, 1, 1], hist[1, 1, 15], hist[0, 0, 3] = 5, 4, 3, 2, 9
    counts = {"hist": hist.reshape(-1).tolist(), "emptied": [2, 1], "stripped": 6, "pairs_dropped": 7, "n_kept": 30, "cols_kept": 999}
    text = ref.report_of(33, counts, False, False).split("\n")
    assert text[0] == "# ma_hip end mask: 33 records, 30 kept, 2 1 emptied, 7 inserts dropped, 6 gap columns stripped, mode trim, library ds"
    assert text[1] == "# k\t5p+\t5p-\t3p+\t3p-"
    assert text[2] == "1\t5\t4\t3\t0" and text[4] == "3\t9\t0\t0\t0" and text[16] == "15\t0\t0\t0\t2"
    assert len(text) == 18 and text[17] == ""
    assert ref.report_of(0, ref.mask(kc.case("empty"), 3, 3, True, True).counts(), True, True).split("\n")[0].endswith("mode N, library ss")
    assert ref.report(kc.case("empty"), 3, 3).split("\n")[2:17] == ["%d\t0\t0\t0\t0" % k for k in range(1, 16)]


def test_cases_hold_what_they_promise():
    assert sum(len(r["seq"]) for r in kc.case("long_5000").rec) % 16 != 0
    m = kc.case("chunk_edge")
    at = [r["id"] for r in m.rec].index("straddle")
    off = sum(len(r["seq"]) for r in m.rec[:at])
    assert off < kc.CHUNK < off + 40
    got = ref.mask(kc.case("all_emptied"), 15, 15)
    assert got.n_kept == 0 and sum(got.emptied) == 60 and got.emptied[0] and got.emptied[1]
    offs = {(int(o) % 16, int(e) % 16) for o, e in zip(ms.flatten(kc.case("offsets"))["col_off"][:-1], ms.flatten(kc.case("offsets"))["col_off"][1:])}
    assert {o for o, _ in offs} == set(range(16)) and {e for _, e in offs} == set(range(16))
    got = ref.mask(kc.case("pairs300"), 3, 3)
    assert len(kc.case("pairs300").rec[0]["ins"]) == 300 and got.pairs_dropped >= 5 and int(got.pair_keep.sum()) > 280
    got = ref.mask(kc.case("dashes"), 3, 3)
    assert got.stripped >= 8 and sum(got.emptied) == 2
    got = ref.mask(kc.case("codes"), 3, 3)
    inner = sum(1 for r in got.maln.rec for c, ch in enumerate(r["smp"]) if ref.zones(ch, r["rc"], 3, 3) != (0, 0))
    assert inner > 100                                       # zone codes between kept columns


@pytest.mark.parametrize("name", ("offsets", "pairs300", "chunk_edge", "dashes"))
def test_trim_commutes_with_the_tally(name):
    """maln_synth's restated tally over the masked Maln equals a tally over the ORIGINAL's arrays without the removed columns and pairs"""
    m = kc.case(name)
    f = ms.flatten(m)
    for n5, n3 in ((3, 3), (15, 15), (5, 0)):
        got = ref.mask(m, n5, n3)
        keep = got.count > 0
        ncols = f["col_off"][1:] - f["col_off"][:-1]
        rec = np.repeat(np.arange(len(m.rec)), ncols)
        c = np.arange(f["col_off"][-1]) - f["col_off"][:-1][rec]
        col_keep = (c >= got.first[rec]) & (c < got.first[rec] + got.count[rec])
        pk = got.pair_keep.astype(bool)
        new_no = np.cumsum(keep) - 1
        ilen = (f["ins_off"][1:] - f["ins_off"][:-1])
        sub = dict(f, gaps=got.maln.gaps, start=got.start[keep], revcom=f["revcom"][keep], col_off=np.concatenate([[0], np.cumsum(got.count[keep])]).astype(np.int64),
                   seq=f["seq"][col_keep], smp=f["smp"][col_keep], ins_record=new_no[f["ins_record"][pk]].astype(np.int32), ins_pos=got.ins_pos[pk],
                   ins_off=np.concatenate([[0], np.cumsum(ilen[pk])]).astype(np.int64), ins_bases=f["ins_bases"][np.repeat(pk, ilen)])
        a = ms.Restated(sub, m.fpsm, m.rpsm, m.ref_seq, m.ref_id)
        b = ms.restate(got.maln)
        assert np.array_equal(a.cols, b.cols) and np.array_equal(a.ins, b.ins) and np.array_equal(a.span, b.span), (name, n5, n3)
        assert a.table(1) == b.table(1)
        assert bytes(f["seq"][col_keep]) == got.seq and bytes(f["smp"][col_keep]) == got.smp


def test_the_restatement_gives_the_recorded_counts():
    import ma_mask_goldens as mg
    with gzip.open(GOLD) as f:
        gold = json.load(f)
    assert sorted(gold["files"]) == sorted(mg.INPUTS)
    for name in mg.INPUTS:
        m = mg.load(name)
        assert sorted(gold["files"][name]) == sorted(ref.tag(*s) for s in ref.SETTINGS)
        for s in ref.SETTINGS:
            assert ref.mask(m, *s).counts() == gold["files"][name][ref.tag(*s)]["counts"], (name, s)
    assert mg.rare_paths(mg.all_masks()) == []


def sanitizer_flags(tmp):
    """-fsanitize=address,undefined if g++ can link and run such a program here, else nothing"""
    src, exe = tmp / "probe.cpp", tmp / "probe"
    src.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    ok = subprocess.run(["g++"] + flags + ["-o", str(exe), str(src)], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode == 0
    return flags if ok and subprocess.run([str(exe)]).returncode == 0 else []


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ma_mask")
    flags = sanitizer_flags(tmp)
    print("ma_mask_driver: sanitizers", "on" if flags else "not available: compiled without")
    exe = tmp / "ma_mask_driver"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-g"] + flags + ["-o", str(exe), os.path.join(ROOT, "tests", "ma_mask_driver.cpp")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()
    return str(exe)


def driver_input(m, path):
    f = ms.flatten(m)
    with open(path, "w", encoding="latin1") as out:
        out.write("%d %d %d\n>%s\n>%s\n" % (len(m.rec), f["col_off"][-1], len(f["ins_pos"]), f["seq"].tobytes().decode("latin1"), f["smp"].tobytes().decode("latin1")))
        for r in range(len(m.rec)):
            out.write("%d %d %d\n" % (f["start"][r], f["revcom"][r], f["col_off"][r + 1]))
        for e in range(len(f["ins_pos"])):
            out.write("%d %d\n" % (f["ins_record"][e], f["ins_pos"][e]))
    return path


@pytest.mark.parametrize("name", kc.CASES)
def test_host_build_of_the_kernels_body_agrees(driver, name, tmp_path):
    m = kc.case(name)
    path = driver_input(m, str(tmp_path / "in.txt"))
    for n5, n3, x, ss in ref.SETTINGS + ((15, 1, False, False), (1, 15, True, True)):
        got = subprocess.run([driver, path, str(n5), str(n3), "1" if x else "0", "1" if ss else "0"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert got.returncode == 0, (n5, n3, x, ss, got.stderr.decode("latin1")[-2000:])
        lines = got.stdout.decode("latin1").split("\n")
        assert len(lines) == 11 and lines[10] == ""
        want = ref.mask(m, n5, n3, x, ss)
        row = lambda k, key: np.array(lines[k].split()[1:], np.int64) if lines[k].split()[0] == key else None
        what = (name, n5, n3, x, ss)
        for k, (key, arr) in enumerate((("first", want.first), ("count", want.count), ("start", want.start), ("col_off", want.col_off))):
            assert np.array_equal(row(k, key), arr), what + (key,)
        assert lines[4] == ">" + want.seq.decode("latin1") and lines[5] == ">" + want.smp.decode("latin1"), what
        assert np.array_equal(row(6, "pair_keep"), want.pair_keep) and np.array_equal(row(7, "ins_pos"), want.ins_pos), what
        c = want.counts()
        assert row(8, "hist").tolist() == c["hist"], what
        assert row(9, "scalars").tolist() == c["emptied"] + [c["stripped"], c["pairs_dropped"], c["n_kept"], c["cols_kept"]], what


def test_mask_symbols_declared_exported_and_bound():
    import mia_amd
    hdr = open(os.path.join(ROOT, "include", "mia_hip.h")).read()
    declared = set(re.findall(r"\b(mia_hip_[a-z_0-9]+)\s*\(", hdr))
    lib = mia_amd.lib()
    for sym in ("mia_hip_ma_mask", "mia_hip_get_ma_mask"):
        assert sym in declared, sym
        assert sym in mia_amd.exported_symbols(), sym
        assert hasattr(lib, sym), sym
    assert hasattr(mia_amd.MiaHip, "ma_mask")
    stages = mia_amd.MiaHip.STAGES
    at = stages.index("k_ma_mask_bounds")
    assert stages[at:at + 3] == ["k_ma_mask_bounds", "k_ma_mask_layout", "k_ma_mask_apply"]
    src = open(os.path.join(ROOT, "mapping-iterative-assembler_amd", "csrc", "mia_hip.hip")).read()
    table = re.search(r"STAGE_NAMES\[STG_COUNT\] = \{(.*?)\};", src, re.S).group(1)
    assert re.findall(r'"([a-z_0-9]+)"', table) == stages
    assert len(stages) <= 32                                 # a bit per stage in mia_hip_set_stage_mask
    for f in ("ma_mask_body.h", "mia_ma_mask_kernels.h"):
        assert os.path.exists(os.path.join(ROOT, "mapping-iterative-assembler_amd", "csrc", f))
