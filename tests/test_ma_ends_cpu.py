"""Fragment-end context (ma_hip -f 92) and read lengths (-f 93) without a GPU.  The reference's `ma` has neither report, so no
recording pins them whole; the rule of tests/ma_ends_ref.py (written from DESIGN.md's text) is tied to the reference in the two places
where it did produce the data: the true ends per column and strand are columns 5-8 of its own `ma -f 3` (tests/golden/ma_ends, made
by tools/make_ma_ends_goldens.py), and a read's length is len(SEQ) of the SAM rule (tests/ma_sam_ref.py).  The code k_ma_ends runs
per lane (csrc/ma_ends_body.h) is compiled for the host into tests/ma_ends_driver.cpp, with -fsanitize=address,undefined where g++ has
that runtime, run as a program of its own, and must make the bins of the restatement."""
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

import ma_ends_ref as ref
import ma_sam_ref as sam_ref
import maln_ace_cases as mc
import maln_ends_cases as ec
import maln_profile_cases as pc
import maln_sam_cases as sc
import maln_synth as ms
from conftest import GOLDEN, ROOT

NAMES = tuple("ends:" + n for n in ec.CASES) + tuple("ace:" + n for n in mc.CASES) + tuple("synth:" + n for n in ms.CASES) + \
    tuple("sam:" + n for n in sc.CASES) + tuple("prof:" + n for n in pc.CASES)
F3_NAMES = tuple("ends:" + n for n in ec.CASES) + ("ace:shapes", "ace:column300") + tuple("ace:" + n for n in mc.FIXTURES) + ("synth:deep",)
_made, _counts = {}, {}


def case(name):
    if name not in _made:
        kind, key = name.split(":", 1)
        _made[name] = {"ends": ec.make_case, "ace": mc.make_case, "synth": ms.make_case, "sam": sc.make_case, "prof": pc.make_case}[kind](key)
    return _made[name]


def counts(name, use_dropped):
    if name not in _counts:
        _counts[name] = ref.counts_split(case(name))
    return ref.counts(case(name), use_dropped, _counts[name])


@pytest.fixture(scope="module")
def f3():
    with open(os.path.join(GOLDEN, "ma_ends", "f3_ends.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("name", F3_NAMES)
def test_true_ends_are_columns_5_to_8_of_the_references_format_3(name, f3):
    """every record, dropped or not, as the reference counts them.  An end on a column that is no reference column (column L of a
    record that ends there, column -1 of one without columns at START 0) has no row in the reference's table."""
    m = case(name)
    gold = f3[name]
    kind, key = name.split(":", 1)
    text = ms.write_maln(ec.for_the_reference(m)) if kind == "ends" else mc.case_text(key) if kind == "ace" else ms.write_maln(m)
    assert hashlib.sha256(text.encode("latin1")).hexdigest() == gold["sha256"], "the recorded run read another file"
    assert gold["records"] == len(m.rec) and gold["rows"] == m.L
    want = {int(c): four for c, four in gold["ends"].items()}
    got = {c: four for c, four in ref.true_ends(m).items() if 0 <= c < m.L}
    assert got == want


@pytest.mark.parametrize("name", NAMES)
def test_length_is_the_length_of_the_sam_rules_seq(name):
    m = case(name)
    for r in m.rec:
        if ref.seg_of(r) not in ("f", "b"):
            assert ref.length(r) == len(sam_ref.walk(r, m.L, m.ref_seq)[1]), (name, r["id"])


@pytest.mark.parametrize("name", NAMES)
def test_sums(name):
    m = case(name)
    for use_dropped in (False, True):
        ctx, lens, halves = counts(name, use_dropped)
        n5, n3 = ref.n_ends(ctx)
        assert (ctx[0].sum(axis=1) == n5).all() and (ctx[1].sum(axis=1) == n3).all()
        used = ref.counted(m, use_dropped)
        assert int(lens.sum()) + halves == len(used)
        assert n5 == sum(1 for r in used if ref.seg_of(r) != ("f" if r["rc"] else "b"))
        assert n3 == sum(1 for r in used if ref.seg_of(r) != ("b" if r["rc"] else "f"))


# hand12: ACGTNACGTacg.  One string per end: the class (A C G T other outside = 0 .. 5) at positions -10 .. -1, +1 .. +10.
#   fwd        columns 2 .. 6, forward:  5' anchor 2: in front columns -8 .. 1, inside 2 .. 11;  3' anchor 6: inside -3 .. 6, behind 7 .. 16
#   rev        columns 5 .. 8, reverse (classes complemented, the read runs down the columns):
#              5' anchor 8: in front columns 18 .. 9, inside 8 .. -1;  3' anchor 5: inside 14 .. 5, behind 4 .. -5
#   back_half  columns 9 .. 11, forward, SEG b: no 5' end;  3' anchor 11: inside 2 .. 11, behind 12 .. 21
HAND12 = {
    0: ["5555555501" "2340123012",         # fwd
        "5555555123" "0123401235"],        # rev
    1: ["5550123401" "2301255555",         # fwd
        "5551230123" "4012355555",         # rev
        "2340123012" "5555555555"],        # back_half
}
HAND12_LENS = {(0, 6): 1, (1, 5): 1}       # fwd: GT-AC and A-C, rev: ACGT and T (the later pair of position 0)


def hand12_counts():
    ctx, lens = np.zeros((2, 20, 6), np.int64), np.zeros((2, 513), np.int64)
    for end, rows in HAND12.items():
        for row in rows:
            assert len(row) == 20
            for o, ch in enumerate(row):
                ctx[end, o, int(ch)] += 1
    for (rc, l), k in HAND12_LENS.items():
        lens[rc, l] = k
    return ctx, lens, 1


def test_hand12_against_its_literal():
    m = case("ends:hand12")
    assert m.ref_seq == "ACGTNACGTacg" and len(m.rec) == 3
    ctx, lens, halves = counts("ends:hand12", False)
    want = hand12_counts()
    assert np.array_equal(ctx, want[0]) and np.array_equal(lens, want[1]) and halves == want[2]
    assert ref.lengths_table(m) == ("# ma_hip read lengths: 2 whole records, 1 halves of reads split at the origin (not counted), 0 longer than 511\n"
                                    "# length\tforward\treverse\n5\t0\t1\n6\t1\t0\n")
    lines = ref.ends_table(m).split("\n")
    assert lines[0] == "# ma_hip fragment ends: 3 records, 2 5' ends, 3 3' ends" and lines[1] == "# end\tposition\tA\tC\tG\tT\tother\toutside"
    assert lines[2] == "5p\t-10\t0\t0\t0\t0\t0\t2" and lines[12] == "5p\t+1\t1\t0\t1\t0\t0\t0" and lines[41] == "3p\t+10\t0\t0\t0\t0\t0\t3" and lines[42:] == [""]


def test_cases_hold_what_they_promise():
    short = case("ends:short_ref")
    assert short.L == 7
    ctx = counts("ends:short_ref", True)[0]
    assert (ctx[:, 0, 5] > 0).all() and (ctx[:, 19, 5] > 0).all()                   # windows leave the reference on both sides
    e = case("ends:edges")
    for rc in (0, 1):
        for seg in "afbn":
            mine = [r for r in e.rec if r["rc"] == rc and r["seg"] == seg]
            assert set(range(11)) <= {r["start"] for r in mine} and set(range(e.L - 11, e.L)) <= {r["end"] for r in mine}
    assert any(r["end"] == e.L for r in e.rec) and int(e.gaps.sum()) >= 1
    assert any(r["end"] == r["start"] - 1 and r["start"] == 450 for r in e.rec) and not any(r["end"] < r["start"] and r["start"] == 0 for r in e.rec)
    c = case("ends:codes")
    assert "N" in c.ref_seq and set("RYKMSWBDHV") <= set(c.ref_seq) and any("a" <= ch <= "z" for ch in c.ref_seq)
    assert (counts("ends:codes", True)[0][:, :, 4] > 0).any(axis=1).all()
    for K in ec.PILES:
        p = case("ends:pile_%d" % K)
        same = [r for r in p.rec if r["id"] != "other"]
        assert len(same) == K and len(p.rec) == K + 1 and len({(r["start"], r["seq"], r["rc"], tuple(r["ins"])) for r in same}) == 1
    assert {63, 64, 65, 255, 256, 257} == set(ec.PILES) and len(case("ends:pile_5000").rec) == 5000
    lens_case = case("ends:lens")
    for rc in (0, 1):
        have = {ref.length(r) for r in lens_case.rec if r["rc"] == rc and ref.seg_of(r) not in ("f", "b")}
        assert set(ec.LENS_WANTED) <= have, rc
    ins = [r["ins"] for r in lens_case.rec]
    assert any(len({p for p, _ in i}) < len(i) for i in ins) and any("-" in s for i in ins for _, s in i)
    assert all(any(p == where(r) for p, _ in r["ins"]) for where in (lambda r: -1, lambda r: r["end"] - r["start"], lambda r: r["end"] - r["start"] + 1)
               for r in lens_case.rec if r["id"] == "l9")
    lens = counts("ends:lens", True)
    assert lens[1][:, 512].tolist() == [3, 3] and lens[2] == 4              # 512, 513 and 700 per strand; f and b per strand


# ---- csrc/ma_ends_body.h on the host ----------------------------------------------------------------------------------------------
def sanitizer_flags(tmp):
    """-fsanitize=address,undefined if a program built with it links and runs here"""
    src, exe = tmp / "probe.cpp", tmp / "probe"
    src.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    ok = subprocess.run(["g++"] + flags + ["-o", str(exe), str(src)], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode == 0
    return flags if ok and subprocess.run([str(exe)]).returncode == 0 else []


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ma_ends")
    flags = sanitizer_flags(tmp)
    print("ma_ends_driver: sanitizers", "on" if flags else "not available: compiled without")
    exe = tmp / "ma_ends_driver"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-g"] + flags + ["-o", str(exe), os.path.join(ROOT, "tests", "ma_ends_driver.cpp")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()
    return str(exe)


def test_dashes_by_words_at_every_offset_and_length(driver):
    got = subprocess.run([driver, "dashes"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert got.returncode == 0, got.stderr.decode("latin1")[-2000:]
    assert int(got.stdout) == 2 * 48 * 81


@pytest.mark.parametrize("name", NAMES)
def test_host_build_of_the_kernels_record_agrees(driver, name, tmp_path):
    m = case(name)
    path = str(tmp_path / "in.maln")
    with open(path, "w", encoding="latin1") as f:
        f.write(ms.MA_HEADER + ms.write_maln(m))
    for use_dropped, back in ((False, False), (True, True)):
        got = subprocess.run([driver, "counts", path] + (["A"] if use_dropped else []) + (["back"] if back else []), stdout=subprocess.PIPE,
                             stderr=subprocess.PIPE, timeout=300)
        assert got.returncode == 0, got.stderr.decode("latin1")[-2000:]
        ctx, lens, halves = counts(name, use_dropped)
        want = [len(ref.counted(m, use_dropped))] + ctx.reshape(-1).tolist() + lens.reshape(-1).tolist() + [halves]
        assert [int(x) for x in got.stdout.split()] == want, (name, use_dropped)


def test_ends_symbols_declared_and_exported():
    import mia_amd
    hdr = open(os.path.join(ROOT, "include", "mia_hip.h")).read()
    declared = set(re.findall(r"\b(mia_hip_[a-z_0-9]+)\s*\(", hdr))
    lib = mia_amd.lib()
    for sym in ("mia_hip_ma_ends", "mia_hip_get_ma_ends"):
        assert sym in declared, sym
        assert sym in mia_amd.exported_symbols(), sym
        assert hasattr(lib, sym), sym
    assert hasattr(mia_amd.MiaHip, "ma_ends")
    assert mia_amd.MiaHip.STAGES[-1] == "k_ma_ends"
    assert os.path.exists(os.path.join(ROOT, "mapping-iterative-assembler_amd", "csrc", "ma_ends_body.h"))
