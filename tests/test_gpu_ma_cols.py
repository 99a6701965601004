"""ma_hip's strand-split column table (-f 42).  The reference's `ma` has no such report: ma_hip must print, byte for byte, the text of
tests/ma_cols_ref.py (the rule of DESIGN.md restated in numpy, which tests/test_ma_cols_cpu.py ties to the reference's own `ma -f 3` and
`-f 41`), and the library call behind it (mia_hip_ma_cols: one launch of k_ma_cols, a tile of reference columns per workgroup in LDS)
must give the same table.  The shapes at which the kernel can go wrong are those of tests/maln_cols_cases.py."""
import copy
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ma_ace_ref as ace_ref
import ma_cols_ref as ref
import maln_ace_cases as mc
import maln_cols_cases as cc
import maln_ends_cases as ec
import maln_profile_cases as pc
import maln_sam_cases as sc
import maln_synth as ms
from conftest import ROOT

pytestmark = pytest.mark.gpu

MA = os.path.join(ROOT, "mapping-iterative-assembler_amd", "ma_hip")
ERR_STATE = -4                             # MIA_HIP_ERR_STATE (include/mia_hip.h)
NAMES = tuple("cols:" + n for n in cc.CASES) + tuple("ends:" + n for n in ec.CASES) + tuple("ace:" + n for n in mc.CASES) + \
    tuple("synth:" + n for n in ms.CASES) + tuple("sam:" + n for n in sc.CASES) + tuple("prof:" + n for n in pc.CASES)
LIBRARY = tuple("cols:" + n for n in cc.CASES + cc.LIBRARY_ONLY) + ("ends:edges", "ends:pile_63", "ends:pile_64", "ends:pile_65", "ends:pile_255",
                                                                    "ends:pile_256", "ends:pile_257", "ends:pile_5000", "ace:shapes", "ace:empty",
                                                                    "synth:edge257", "synth:scan16_4097", "synth:deep")
_made, _counts = {}, {}


def case(name):
    if name not in _made:
        kind, key = name.split(":", 1)
        _made[name] = {"cols": cc.make_case, "ends": ec.make_case, "ace": mc.make_case, "synth": ms.make_case, "sam": sc.make_case,
                       "prof": pc.make_case}[kind](key)
    return _made[name]


def counts(name, use_dropped):
    """the restatement's table, made once per case"""
    if (name, use_dropped) not in _counts:
        _counts[name, use_dropped] = ref.counts(case(name), use_dropped)
    return _counts[name, use_dropped]


def write(m, path):
    with open(path, "w", encoding="latin1") as f:
        f.write(ms.MA_HEADER + ms.write_maln(m))
    return path


def ma_hip(path, args):
    return subprocess.run([MA, "-M", path] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


def same_text(name, raw, want):
    want = want.encode("latin1")
    if raw != want:
        a, b = raw.split(b"\n"), want.split(b"\n")
        at = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        pytest.fail(f"{name}: line {at + 1}: {a[at:at + 1]!r} instead of {b[at:at + 1]!r}")


@pytest.mark.parametrize("name", NAMES)
def test_report_identical(name, tmp_path):
    m = case(name)
    path = write(m, str(tmp_path / "in.maln"))
    cut = cc.cutting_region(m)
    for args, want in ((["-f", "42"], lambda: ref.report(m, False, counts(name, False))),
                       (["-f", "42", "-A", "-I", "x", "-c", "2", "-R", cut],                    # (-I and -c have no effect; the counts are the whole file's)
                        lambda: ref.report(m, True, counts(name, True), ref.region(cut, m.L)))):
        r = ma_hip(path, args)
        assert r.returncode == 0, (args, r.stderr[-300:])
        same_text("%s %s" % (name, " ".join(args)), r.stdout, want())


def test_regions_as_format_6_reads_them(tmp_path):
    m = case("cols:hand")
    path = write(m, str(tmp_path / "in.maln"))
    for text in ("4:5", "9:3", "0:99", "13:20", "12:12"):       # inside; start > end: both the smaller; clamped; empty: the two header lines; one row
        r = ma_hip(path, ["-f", "42", "-R", text])
        assert r.returncode == 0, (text, r.stderr[-300:])
        same_text("hand -R " + text, r.stdout, ref.report(m, False, counts("cols:hand", False), ref.region(text, m.L)))


def test_report_and_rewrite_in_one_run(tmp_path):
    m = case("ace:shapes")
    path, out = write(m, str(tmp_path / "in.maln")), str(tmp_path / "out.maln")
    r = ma_hip(path, ["-f", "42", "-c", "2", "-I", "my_contig", "-m", out])
    assert r.returncode == 0, r.stderr[-300:]
    same_text("shapes -f 42 -m", r.stdout, ref.report(m, False, counts("ace:shapes", False)))
    with open(out, "rb") as f:
        same_text("shapes -m file", f.read().split(b"\n", 1)[1], ace_ref.rewrite(m, 2, "my_contig"))


def test_formats_3_and_94_are_still_refused_and_the_help_names_42(tmp_path):
    path = write(case("cols:hand"), str(tmp_path / "in.maln"))
    for fmt in ("3", "94"):
        r = ma_hip(path, ["-f", fmt])
        assert r.returncode != 0 and b"outside the MI355X-accelerated path" in r.stderr and b"42" in r.stderr and b"92" in r.stderr and r.stdout == b""
    r = subprocess.run([MA], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert b"41, 42, 5" in r.stdout and b"-f 42" in r.stdout


# ---- the library call ------------------------------------------------------------------------------------------------------------
def tally(hip, m):
    """the records in the order of m.rec, whatever their START"""
    hip.set_pssm(m.fpsm, m.rpsm)
    hip.ma_tally(*ms.ma_tally_args(ms.flatten(m)))


def use_of(m):
    return np.array([0 if r["dr"] else 1 for r in m.rec], np.uint8)


def seg_of(m):
    return "".join(ref.seg_of(r) for r in m.rec)


def check(got, want, what):
    cols = got[0]
    assert cols.dtype == np.int32 and cols.shape == want[0].shape, what
    if not np.array_equal(cols, want[0]):
        w, p = [int(x[0]) for x in np.nonzero(cols != want[0])]
        pytest.fail(f"{what}: word {w} ({ref.NAMES[w]}) of column {p} = {cols[w, p]}, not {want[0][w, p]}")
    assert tuple(got[1:]) == tuple(want[1:]), what


def shuffled(m, seed):
    t = copy.copy(m)
    order = np.random.RandomState(seed).permutation(len(m.rec))
    t.rec = [m.rec[int(i)] for i in order]
    return t


def all_whole(m):
    t = copy.copy(m)
    t.rec = [dict(r, seg="n") for r in m.rec]
    return t


@pytest.mark.parametrize("name", LIBRARY)
def test_library_call_matches_the_restatement(name):
    import mia_amd
    hip = mia_amd.MiaHip(0)
    m = case(name)
    tally(hip, m)
    hip.stage_stats(reset=True)
    check(hip.ma_cols(seg_of(m), use_of(m)), counts(name, False), name + " (use given)")
    check(hip.ma_cols(seg_of(m)), counts(name, True), name + " (use NULL)")
    check(hip.ma_cols(None, use_of(m)), ref.counts(all_whole(m), False), name + " (segment NULL)")
    st = hip.stage_stats()
    assert st["k_ma_cols"][1] == (3 if m.rec else 0)                       # one launch per call, none without records
    # the same records in another order: the same table; and through the same context, behind a new tally
    back = shuffled(m, 42)
    tally(hip, back)
    check(hip.ma_cols(seg_of(back), use_of(back)), counts(name, False), name + " (shuffled)")
    sel = np.arange(len(m.rec)) % 3 != 1                                   # a mask of its own: every third record left out
    part = copy.copy(back)
    part.rec = [r for r, keep in zip(back.rec, sel.tolist()) if keep]
    check(hip.ma_cols(seg_of(back), sel.astype(np.uint8)), ref.table(m.L, part.rec), name + " (every third left out)")


def test_jobs_of_other_sizes_and_the_other_reports_through_one_context():
    """large, small, larger, none, small: the buffers grow and are used again; the profile and the fragment ends, which share the
    selection's and the segments' buffers, and the SAM export before and after"""
    import mia_amd
    hip = mia_amd.MiaHip(0)
    for name in ("ends:pile_5000", "cols:hand", "synth:deep", "ace:empty", "cols:tile_m1"):
        m = case(name)
        tally(hip, m)
        others = lambda: hip.ma_profile(m.ref_seq, use_of(m))[:2] + hip.ma_ends(m.ref_seq, seg_of(m), use_of(m))[:2] + hip.ma_sam(m.ref_seq)
        before = others()
        hip.stage_stats(reset=True)
        check(hip.ma_cols(seg_of(m), use_of(m)), counts(name, False), name)
        check(hip.ma_cols(seg_of(m), use_of(m)), counts(name, False), name + " (again)")
        st = hip.stage_stats(reset=True)
        assert st["k_ma_cols"][1] == (2 if m.rec else 0)                  # the same launch count for a repeated call
        after = others()
        assert len(before) == len(after) and all(np.array_equal(a, b) for a, b in zip(before, after)), name
        print("%s: %d records; k_ma_cols %.3f ms (two calls)" % (name, len(m.rec), st["k_ma_cols"][0]))


def test_call_order_and_refusal():
    import mia_amd
    hip = mia_amd.MiaHip(0)
    n = C.c_int64()
    assert hip._l.mia_hip_ma_cols(hip._h, None, None, C.byref(n), None, None, None) == ERR_STATE            # no tally yet
    assert hip._l.mia_hip_get_ma_cols(hip._h, None) == ERR_STATE
    good = case("cols:tile_p1")
    tally(hip, good)
    assert hip._l.mia_hip_get_ma_cols(hip._h, None) == ERR_STATE                                            # tallied, no call yet
    check(hip.ma_cols(seg_of(good), use_of(good)), counts("cols:tile_p1", False), "tile_p1 after the refusals")
    assert hip._l.mia_hip_ma_cols(hip._h, None, None, None, None, None, None) == 0                          # every pointer may be NULL
    assert hip._l.mia_hip_get_ma_cols(hip._h, None) == 0                                                    # the getter's too
    other = case("cols:outside")
    tally(hip, other)
    assert hip._l.mia_hip_get_ma_cols(hip._h, None) == ERR_STATE                                            # a new tally: no table yet
    check(hip.ma_cols(seg_of(other), use_of(other)), counts("cols:outside", False), "outside after the refusals")
