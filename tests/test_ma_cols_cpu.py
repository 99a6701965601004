"""The strand-split column table (ma_hip -f 42) without a GPU.  The rule of tests/ma_cols_ref.py (written from DESIGN.md's text) is
tied to the reference in two places: its words 12 .. 15 are columns 5-8 of the reference's own `ma -f 3` (tests/golden/ma_ends, made by
tools/make_ma_ends_goldens.py), and its words 0 .. 11, added over the two strands, are coverage, A, C, G, T and gaps of
maln_synth.restate, which tests/test_ma_synth_cpu.py pins to the reference's recorded `-f 41`.  The code k_ma_cols runs per record
and tile (csrc/ma_cols_body.h) is compiled for the host into tests/ma_cols_driver.cpp, with -fsanitize=address,undefined where g++
has that runtime, run as a program of its own, and must make the table of the restatement."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import ma_cols_ref as ref
import maln_ace_cases as mc
import maln_cols_cases as cc
import maln_ends_cases as ec
import maln_profile_cases as pc
import maln_sam_cases as sc
import maln_synth as ms
from conftest import GOLDEN, ROOT

NAMES = tuple("cols:" + n for n in cc.CASES) + tuple("ends:" + n for n in ec.CASES) + tuple("ace:" + n for n in mc.CASES) + \
    tuple("synth:" + n for n in ms.CASES) + tuple("sam:" + n for n in sc.CASES) + tuple("prof:" + n for n in pc.CASES)
_made, _counts = {}, {}


def case(name):
    if name not in _made:
        kind, key = name.split(":", 1)
        _made[name] = {"cols": cc.make_case, "ends": ec.make_case, "ace": mc.make_case, "synth": ms.make_case, "sam": sc.make_case,
                       "prof": pc.make_case}[kind](key)
    return _made[name]


def counts(name, use_dropped):
    if (name, use_dropped) not in _counts:
        _counts[name, use_dropped] = ref.counts(case(name), use_dropped)
    return _counts[name, use_dropped]


with open(os.path.join(GOLDEN, "ma_ends", "f3_ends.json")) as _f:
    F3 = json.load(_f)


@pytest.mark.parametrize("name", sorted(F3))
def test_words_12_to_15_are_columns_5_to_8_of_the_references_format_3(name):
    """every record, dropped or not, as the reference counts them; zero where the recording lists nothing"""
    m = case(name)
    gold = F3[name]
    assert gold["records"] == len(m.rec) and gold["rows"] == m.L
    want = np.zeros((4, m.L), np.int64)
    for col, four in gold["ends"].items():
        want[:, int(col)] = four
    assert np.array_equal(counts(name, True)[0][12:16], want)


@pytest.mark.parametrize("key", tuple(ms.CASES))
def test_strand_sums_are_the_counts_of_format_41(key):
    m = case("synth:" + key)
    cols = counts("synth:" + key, True)[0]
    both = cols[0:6] + cols[6:12]
    r = ms.restate(m)
    for w, word in enumerate(("A", "C", "G", "T", "gaps")):
        assert np.array_equal(both[w], r.cols[ms.COL_WORDS.index(word)]), word
    assert np.array_equal(both.sum(axis=0), r.cols[ms.COL_WORDS.index("cov")])


# hand: ACGTNACGTacg.  {column: {word: count}}; words 0 .. 5 = A C G T gap other of forward records, 6 .. 11 of reverse ones,
# 12, 13 = forward / reverse starts, 14, 15 = forward / reverse ends.
#   fwd         CGTT  on columns 1 .. 4, forward, whole            rev         TNAC  on columns 3 .. 6, reverse, whole
#   back_half   TAC   on columns 8 .. 10, forward, SEG b: no start  front_half  g-NA  on columns 7 .. 10, reverse, SEG f: no end
HAND = {
    1: {1: 1, 12: 1},
    2: {2: 1},
    3: {3: 1, 9: 1, 13: 1},
    4: {3: 1, 11: 1, 14: 1},
    5: {6: 1},
    6: {7: 1, 15: 1},
    7: {11: 1, 13: 1},
    8: {3: 1, 10: 1},
    9: {0: 1, 11: 1},
    10: {1: 1, 6: 1, 14: 1},
}


def hand_table():
    cols = np.zeros((16, 12), np.int64)
    for p, words in HAND.items():
        for w, k in words.items():
            cols[w, p] = k
    return cols


def test_hand_against_its_literal():
    m = case("cols:hand")
    assert m.ref_seq == "ACGTNACGTacg" and len(m.rec) == 4
    cols, n_used, n_events, beyond, outside = counts("cols:hand", False)
    assert np.array_equal(cols, hand_table()) and (n_used, n_events, beyond, outside) == (4, 15, 0, 0)
    lines = ref.report(m).split("\n")
    assert lines[0] == "# ma_hip strand table: 4 records, 15 columns, 0 beyond the reference, 0 ends outside it"
    assert lines[1] == "# position\treference\tA+\tC+\tG+\tT+\tgap+\tother+\tA-\tC-\tG-\tT-\tgap-\tother-\tstarts+\tstarts-\tends+\tends-"
    assert lines[2] == "1\tA" + "\t0" * 16 and lines[5] == "4\tT\t0\t0\t0\t1\t0\t0\t0\t0\t0\t1\t0\t0\t0\t1\t0\t0"
    assert lines[12] == "11\tc\t0\t1\t0\t0\t0\t0\t1\t0\t0\t0\t0\t0\t0\t0\t1\t0" and lines[14:] == [""]
    assert ref.report(m, rows=ref.region("4:5", 12)).split("\n")[2:] == lines[5:7] + [""]
    assert ref.region("9:3", 12) == (2, 2) and ref.region("0:99", 12) == (0, 11)                 # the swap that is none; the clamp
    first, last = ref.region("13:20", 12)
    assert first > last and ref.report(m, rows=(first, last)).split("\n")[2:] == [""]


def test_cases_hold_what_they_promise():
    T = cc.T
    assert [case("cols:" + n).L for n in ("tile_m1", "tile_0", "tile_p1")] == [T - 1, T, T + 1]
    for n in ("tile_m1", "tile_0", "tile_p1"):
        m = case("cols:" + n)
        assert {0, 1} == {r["rc"] for r in m.rec if r["end"] == m.L - 1} and any(r["dr"] for r in m.rec)
    e = case("cols:tile_edges")
    assert e.L == 3 * T + 1
    for rc in (0, 1):
        for seg in "afbn":
            mine = [(r["start"], r["end"]) for r in e.rec if r["rc"] == rc and r["seg"] == seg]
            assert any(b == T - 1 and a < b - 1 for a, b in mine) and any(a == T and b > a + 1 for a, b in mine) and (T - 1, T) in mine
            assert any(b - a + 1 == 2 * T + 2 and a // T == 0 and b // T == 2 for a, b in mine)
            assert any(a == 0 for a, b in mine) and any(b == e.L - 1 for a, b in mine)
    o = case("cols:outside")
    assert any(r["start"] == 0 and r["end"] == -1 and not r["rc"] and r["seg"] == "n" for r in o.rec)
    assert {0, 1} <= {r["rc"] for r in o.rec if r["end"] == o.L and not r["dr"]}
    kept, every = counts("cols:outside", False), counts("cols:outside", True)
    assert (kept[3], kept[4]) == (3, 3) and (every[3], every[4]) == (4, 4)       # beyond: the records that end on L; outside: -1 and the ends on L
    t = case("cols:tile_edges")
    assert {"-", "N"} <= set("".join(r["seq"] for r in t.rec)) and any("a" <= ch <= "z" for r in t.rec for ch in r["seq"])


def test_pile_70000_holds_what_it_promises():
    """a pile deeper than 16 bits' worth of records, two forward to one reverse"""
    m = cc.make_case("pile_70000")
    cols, n_used, n_events, beyond, outside = ref.counts(m, True)
    fwd, rev = sum(1 for r in m.rec if r["id"] != "other" and not r["rc"]), sum(1 for r in m.rec if r["id"] != "other" and r["rc"])
    assert fwd + rev == cc.PILE == 70000 > 65536 and fwd == 2 * rev + 1
    assert cols[0, 10] == fwd and cols[1, 11] == fwd and cols[4, 12] == fwd and cols[6, 10] == rev and cols[12, 10] == fwd and cols[15, 12] == rev
    assert (n_used, n_events, beyond, outside) == (70001, 3 * 70000 + 5, 0, 0)


# ---- csrc/ma_cols_body.h on the host ----------------------------------------------------------------------------------------------
def sanitizer_flags(tmp):
    """-fsanitize=address,undefined if a program built with it links and runs here"""
    src, exe = tmp / "probe.cpp", tmp / "probe"
    src.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    ok = subprocess.run(["g++"] + flags + ["-o", str(exe), str(src)], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode == 0
    return flags if ok and subprocess.run([str(exe)]).returncode == 0 else []


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ma_cols")
    flags = sanitizer_flags(tmp)
    print("ma_cols_driver: sanitizers", "on" if flags else "not available: compiled without")
    exe = tmp / "ma_cols_driver"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-g"] + flags + ["-o", str(exe), os.path.join(ROOT, "tests", "ma_cols_driver.cpp")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()
    return str(exe)


@pytest.mark.parametrize("name", NAMES)
def test_host_build_of_the_kernels_body_agrees(driver, name, tmp_path):
    m = case(name)
    path = str(tmp_path / "in.maln")
    with open(path, "w", encoding="latin1") as f:
        f.write(ms.MA_HEADER + ms.write_maln(m))
    for use_dropped, back in ((False, False), (True, True)):
        got = subprocess.run([driver, path] + (["A"] if use_dropped else []) + (["back"] if back else []), stdout=subprocess.PIPE,
                             stderr=subprocess.PIPE, timeout=300)
        assert got.returncode == 0, got.stderr.decode("latin1")[-2000:]
        cols, n_used, n_events, beyond, outside = counts(name, use_dropped)
        assert np.array_equal(np.array(got.stdout.split(), np.int64), np.concatenate([[n_used, n_events, beyond, outside], cols.reshape(-1)])), (name, use_dropped)


def test_cols_symbols_declared_exported_and_bound():
    import mia_amd
    hdr = open(os.path.join(ROOT, "include", "mia_hip.h")).read()
    declared = set(re.findall(r"\b(mia_hip_[a-z_0-9]+)\s*\(", hdr))
    lib = mia_amd.lib()
    for sym in ("mia_hip_ma_cols", "mia_hip_get_ma_cols"):
        assert sym in declared, sym
        assert sym in mia_amd.exported_symbols(), sym
        assert hasattr(lib, sym), sym
    assert hasattr(mia_amd.MiaHip, "ma_cols")
    mine = [s for s in mia_amd.MiaHip.STAGES if s.startswith("k_ma_cols")]
    assert mine == ["k_ma_cols"]
    at = mia_amd.MiaHip.STAGES.index("k_ma_cols")
    assert mia_amd.MiaHip.STAGES[at - 1] == "k_ma_tally" and mia_amd.MiaHip.STAGES[at + 1:] == ["k_ma_ends"]
    # the library's own order: the name table of csrc/mia_hip.hip
    src = open(os.path.join(ROOT, "mapping-iterative-assembler_amd", "csrc", "mia_hip.hip")).read()
    table = re.search(r"STAGE_NAMES\[STG_COUNT\] = \{(.*?)\};", src, re.S).group(1)
    assert re.findall(r'"([a-z_0-9]+)"', table) == mia_amd.MiaHip.STAGES
    for f in ("ma_cols_body.h", "mia_ma_cols_kernels.h"):
        assert os.path.exists(os.path.join(ROOT, "mapping-iterative-assembler_amd", "csrc", f))
