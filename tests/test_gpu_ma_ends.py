"""ma_hip's fragment-end context (-f 92) and read lengths (-f 93).  The reference's `ma` has neither report: ma_hip must print, byte for
byte, the texts of tests/ma_ends_ref.py (the rule of DESIGN.md restated in Python, which tests/test_ma_ends_cpu.py ties to the
reference's own `ma -f 3` and to the SAM rule), and the library call behind it (mia_hip_ma_ends: one launch of k_ma_ends, a record per
lane) must give the same counts.  The shapes at which the kernel can go wrong are those of tests/maln_ends_cases.py."""
import copy
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ma_ace_ref as ace_ref
import ma_ends_ref as ref
import maln_ace_cases as mc
import maln_ends_cases as ec
import maln_profile_cases as pc
import maln_sam_cases as sc
import maln_synth as ms
from conftest import ROOT

pytestmark = pytest.mark.gpu

MA = os.path.join(ROOT, "mapping-iterative-assembler_amd", "ma_hip")
ERR_ARG, ERR_STATE = -2, -4                # MIA_HIP_ERR_ARG, MIA_HIP_ERR_STATE (include/mia_hip.h)
NAMES = tuple("ends:" + n for n in ec.CASES) + tuple("ace:" + n for n in mc.CASES) + tuple("synth:" + n for n in ms.CASES) + \
    tuple("sam:" + n for n in sc.CASES) + tuple("prof:" + n for n in pc.CASES)
LIBRARY = ("ends:hand12", "ends:short_ref", "ends:edges", "ends:codes", "ends:pile_64", "ends:pile_257", "ends:pile_5000", "ends:lens", "ace:shapes",
           "ace:empty", "synth:edge257", "sam:sam_shapes")
_made, _split = {}, {}


def case(name):
    if name not in _made:
        kind, key = name.split(":", 1)
        _made[name] = {"ends": ec.make_case, "ace": mc.make_case, "synth": ms.make_case, "sam": sc.make_case, "prof": pc.make_case}[kind](key)
    return _made[name]


def counts(name, use_dropped):
    """the restatement's counts, made once per case"""
    if name not in _split:
        _split[name] = ref.counts_split(case(name))
    return ref.counts(case(name), use_dropped, _split[name])


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
def test_reports_identical(name, tmp_path):
    m = case(name)
    path = write(m, str(tmp_path / "in.maln"))
    for args, want in ((["-f", "92"], lambda: ref.ends_table(m, False, counts(name, False))),
                       (["-f", "92", "-A", "-I", "x", "-c", "2"], lambda: ref.ends_table(m, True, counts(name, True))),       # (-I and -c have no effect)
                       (["-f", "93", "-I", "x", "-c", "2"], lambda: ref.lengths_table(m, False, counts(name, False))),
                       (["-f", "93", "-A"], lambda: ref.lengths_table(m, True, counts(name, True)))):
        r = ma_hip(path, args)
        assert r.returncode == 0, (args, r.stderr[-300:])
        same_text("%s %s" % (name, " ".join(args)), r.stdout, want())


@pytest.mark.parametrize("fmt", ["92", "93"])
def test_report_and_rewrite_in_one_run(fmt, tmp_path):
    m = case("ace:shapes")
    path, out = write(m, str(tmp_path / "in.maln")), str(tmp_path / "out.maln")
    r = ma_hip(path, ["-f", fmt, "-c", "2", "-I", "my_contig", "-m", out])
    assert r.returncode == 0, r.stderr[-300:]
    table = ref.ends_table if fmt == "92" else ref.lengths_table
    same_text("shapes -f %s -m" % fmt, r.stdout, table(m, False, counts("ace:shapes", False)))
    with open(out, "rb") as f:
        same_text("shapes -m file", f.read().split(b"\n", 1)[1], ace_ref.rewrite(m, 2, "my_contig"))


def test_format_3_is_still_refused_and_the_help_names_the_reports(tmp_path):
    path = write(case("ends:hand12"), str(tmp_path / "in.maln"))
    r = ma_hip(path, ["-f", "3"])
    assert r.returncode != 0 and b"outside the MI355X-accelerated path" in r.stderr and b"92" in r.stderr and r.stdout == b""
    r = ma_hip(path, ["-f", "94"])
    assert r.returncode != 0 and b"outside the MI355X-accelerated path" in r.stderr and r.stdout == b""
    r = subprocess.run([MA], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert b"92" in r.stdout and b"93" in r.stdout


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
    ctx, lens, halves = got
    assert ctx.dtype == np.int64 and ctx.shape == (2, 20, 6) and lens.dtype == np.int64 and lens.shape == (2, 513)
    if not np.array_equal(ctx, want[0]):
        e, o, c = [int(x[0]) for x in np.nonzero(ctx != want[0])]
        pytest.fail(f"{what}: ctx[{e}][{o}][{c}] = {ctx[e, o, c]}, not {want[0][e, o, c]}")
    if not np.array_equal(lens, want[1]):
        rc, l = [int(x[0]) for x in np.nonzero(lens != want[1])]
        pytest.fail(f"{what}: len_count[{rc}][{l}] = {lens[rc, l]}, not {want[1][rc, l]}")
    assert halves == want[2], what


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
    check(hip.ma_ends(m.ref_seq, seg_of(m), use_of(m)), counts(name, False), name + " (use given)")
    check(hip.ma_ends(m.ref_seq, seg_of(m)), counts(name, True), name + " (use NULL)")
    check(hip.ma_ends(m.ref_seq, None, use_of(m)), ref.counts(all_whole(m), False), name + " (segment NULL)")
    st = hip.stage_stats()
    assert st["k_ma_ends"][1] == (3 if m.rec else 0)                       # one launch per call, none without records
    n_used, n5, n3 = C.c_int64(), C.c_int64(), C.c_int64()
    use, seg = use_of(m), np.frombuffer(seg_of(m).encode("latin1"), np.uint8)
    assert hip._l.mia_hip_ma_ends(hip._h, C.c_char_p(m.ref_seq.encode("latin1")), seg.ctypes.data_as(C.c_void_p) if seg.size else None,
                                  use.ctypes.data_as(C.c_void_p) if use.size else None, C.byref(n_used), C.byref(n5), C.byref(n3)) == 0
    assert (n_used.value, (n5.value, n3.value)) == (len(ref.counted(m)), ref.n_ends(counts(name, False)[0]))
    # the same records in another order: the same counts; and through the same context, behind a new tally
    back = shuffled(m, 92)
    tally(hip, back)
    check(hip.ma_ends(back.ref_seq, seg_of(back), use_of(back)), counts(name, False), name + " (shuffled)")
    sel = np.arange(len(m.rec)) % 3 != 1                                   # a mask of its own: every third record left out
    part = copy.copy(back)
    part.rec = [r for r, keep in zip(back.rec, sel.tolist()) if keep]
    check(hip.ma_ends(back.ref_seq, seg_of(back), sel.astype(np.uint8)), ref.counts(part, True), name + " (every third left out)")


def test_jobs_of_other_sizes_and_the_other_reports_through_one_context():
    """large, small, larger, none, small: the buffers grow and are used again; the profile, which shares the reference's and the
    selection's buffers, before and after"""
    import mia_amd
    hip = mia_amd.MiaHip(0)
    for name in ("ends:pile_5000", "ends:hand12", "synth:edge257", "ace:empty", "ends:short_ref"):
        m = case(name)
        tally(hip, m)
        before = hip.ma_profile(m.ref_seq, use_of(m))[:2] + hip.ma_sam(m.ref_seq)
        hip.stage_stats(reset=True)
        check(hip.ma_ends(m.ref_seq, seg_of(m), use_of(m)), counts(name, False), name)
        check(hip.ma_ends(m.ref_seq, seg_of(m), use_of(m)), counts(name, False), name + " (again)")
        st = hip.stage_stats(reset=True)
        assert st["k_ma_ends"][1] == (2 if m.rec else 0)
        after = hip.ma_profile(m.ref_seq, use_of(m))[:2] + hip.ma_sam(m.ref_seq)
        assert len(before) == len(after) and all(np.array_equal(a, b) for a, b in zip(before, after)), name
        print("%s: %d records; k_ma_ends %.3f ms (two calls)" % (name, len(m.rec), st["k_ma_ends"][0]))


def test_call_order_and_refusal():
    import mia_amd
    hip = mia_amd.MiaHip(0)
    n = C.c_int64()
    good = case("ends:edges")
    seq = C.c_char_p(good.ref_seq.encode("latin1"))
    assert hip._l.mia_hip_ma_ends(hip._h, seq, None, None, C.byref(n), None, None) == ERR_STATE             # no tally yet
    assert hip._l.mia_hip_get_ma_ends(hip._h, None, None, None) == ERR_STATE
    tally(hip, good)
    assert hip._l.mia_hip_get_ma_ends(hip._h, None, None, None) == ERR_STATE                                # tallied, no call yet
    assert hip._l.mia_hip_ma_ends(hip._h, None, None, None, C.byref(n), None, None) == ERR_ARG              # no reference
    assert hip._l.mia_hip_get_ma_ends(hip._h, None, None, None) == ERR_STATE
    check(hip.ma_ends(good.ref_seq, seg_of(good), use_of(good)), counts("ends:edges", False), "edges after a refusal")
    assert hip._l.mia_hip_ma_ends(hip._h, seq, None, None, None, None, None) == 0                            # every count may be NULL
    assert hip._l.mia_hip_get_ma_ends(hip._h, None, None, None) == 0                                         # every pointer of the getter too
    other = case("ends:lens")
    tally(hip, other)
    assert hip._l.mia_hip_get_ma_ends(hip._h, None, None, None) == ERR_STATE                                # a new tally: no counts yet
    check(hip.ma_ends(other.ref_seq, seg_of(other), use_of(other)), counts("ends:lens", False), "lens after the refusals")
