"""ma_hip's substitution profile (-f 9 the table, -f 91 a matrix for mia -s).  The reference's `ma` has no such report, so nothing
recorded from it pins this one: ma_hip must print, byte for byte, the texts of tests/ma_profile_ref.py (the rule of DESIGN.md
restated in Python, which tests/test_ma_profile_cpu.py holds to the tally the reference's own `ma -f 41` pins), and the library call
behind it (mia_hip_ma_profile: one launch of k_ma_profile over the flat columns) must give the same counts.  The shapes at which the
kernel can go wrong are those of tests/maln_profile_cases.py.  (The restatement is a plain Python loop over every column: the deepest
case of maln_synth, 2.8 million columns, takes it a few seconds.)"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ma_ace_ref as ace_ref
import ma_profile_ref as ref
import maln_ace_cases as mc
import maln_profile_cases as pc
import maln_sam_cases as sc
import maln_synth as ms
from conftest import ROOT

pytestmark = pytest.mark.gpu

MA = os.path.join(ROOT, "mapping-iterative-assembler_amd", "ma_hip")
ERR_ARG, ERR_STATE = -2, -4                # MIA_HIP_ERR_ARG, MIA_HIP_ERR_STATE (include/mia_hip.h)
# the profile's own shapes, the ACE cases (three of them committed .maln), the ten cases of maln_synth, the SAM shapes
NAMES = tuple("prof:" + n for n in pc.CASES) + tuple("ace:" + n for n in mc.CASES) + tuple("synth:" + n for n in ms.CASES) + tuple("sam:" + n for n in sc.CASES)
_made, _split = {}, {}


def case(name):
    if name not in _made:
        kind, key = name.split(":", 1)
        _made[name] = {"ace": mc.make_case, "synth": ms.make_case, "sam": sc.make_case, "prof": pc.make_case}[kind](key)
    return _made[name]


def prof(name, use_dropped):
    """the restatement's counts, made once per case"""
    if name not in _split:
        _split[name] = ref.profile_split(case(name))
    return ref.profile(case(name), use_dropped, _split[name])


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
def test_profile_identical(name, tmp_path):
    m = case(name)
    path = write(m, str(tmp_path / "in.maln"))
    for args, want in ((["-f", "9"], lambda: ref.table(m, False, prof(name, False))),
                       (["-f", "9", "-A", "-I", "my_contig"], lambda: ref.table(m, True, prof(name, True))),      # (-I has no effect)
                       (["-f", "91"], lambda: ref.matrix(m, 1.0, False, prof(name, False))),
                       (["-f", "91", "-P", "0.25"], lambda: ref.matrix(m, 0.25, False, prof(name, False)))):
        r = ma_hip(path, args)
        assert r.returncode == 0, (args, r.stderr[-300:])
        same_text("%s %s" % (name, " ".join(args)), r.stdout, want())


@pytest.mark.parametrize("value", ["0", "-1", "nan", "inf", "x", "1e-61"])
def test_pseudocount_that_is_refused(value, tmp_path):
    path = write(case("prof:prof_edges_65"), str(tmp_path / "in.maln"))
    r = ma_hip(path, ["-f", "91", "-P", value])
    assert r.returncode == 1 and r.stdout == b"" and len(r.stderr.strip().split(b"\n")) == 1


def test_profile_and_rewrite_in_one_run(tmp_path):
    m = case("ace:shapes")
    path, out = write(m, str(tmp_path / "in.maln")), str(tmp_path / "out.maln")
    r = ma_hip(path, ["-f", "9", "-c", "2", "-I", "my_contig", "-m", out])
    assert r.returncode == 0, r.stderr[-300:]
    same_text("shapes -f 9 -m", r.stdout, ref.table(m, False, prof("ace:shapes", False)))
    with open(out, "rb") as f:
        same_text("shapes -m file", f.read().split(b"\n", 1)[1], ace_ref.rewrite(m, 2, "my_contig"))


def test_format_3_is_still_refused_and_a_bad_code_on_a_base_still_stops_the_tally(tmp_path):
    path = write(case("prof:prof_edges_65"), str(tmp_path / "in.maln"))
    r = ma_hip(path, ["-f", "3"])
    assert r.returncode != 0 and b"outside the MI355X-accelerated path" in r.stderr and r.stdout == b""
    r = ma_hip(write(pc.bad_on_base(), str(tmp_path / "bad.maln")), ["-f", "9"])
    assert r.returncode == 1 and r.stdout == b"" and b"ma_tally" in r.stderr


# ---- the library call ------------------------------------------------------------------------------------------------------------
def tally(hip, m):
    """the records in file order, whatever their START"""
    hip.set_pssm(m.fpsm, m.rpsm)
    hip.ma_tally(*ms.ma_tally_args(ms.flatten(m)))


def use_of(m):
    return np.array([0 if r["dr"] else 1 for r in m.rec], np.uint8)


def check_profile(hip, m, name, want_kept, want_all):
    for use, want in ((use_of(m), want_kept), (None, want_all)):
        count, dele, bad, beyond = hip.ma_profile(m.ref_seq, use)
        assert count.dtype == np.int64 and count.shape == (31, 5, 5) and dele.shape == (31,)
        if not np.array_equal(count, want[0]):
            d, i, j = [int(x[0]) for x in np.nonzero(count != want[0])]
            pytest.fail(f"{name}: count[{d}][{i}][{j}] = {count[d, i, j]}, not {want[0][d, i, j]} (use {'given' if use is not None else 'NULL'})")
        assert np.array_equal(dele, want[1]) and (bad, beyond) == (want[2], want[3]), name


@pytest.mark.parametrize("name", tuple("prof:" + n for n in pc.LIBRARY) + ("synth:edge257", "ace:column300", "sam:sam_4097"))
def test_library_call_matches_the_restatement(name):
    import mia_amd
    hip = mia_amd.MiaHip(0)
    m = case(name)
    tally(hip, m)
    hip.stage_stats(reset=True)
    check_profile(hip, m, name, prof(name, False), prof(name, True))
    st = hip.stage_stats()
    assert st["k_ma_profile"][1] == (2 if m.rec else 0)                    # one launch per call, none without records
    n_used, n_events = C.c_int64(), C.c_int64()
    use = use_of(m)
    assert hip._l.mia_hip_ma_profile(hip._h, C.c_char_p(m.ref_seq.encode("latin1")), use.ctypes.data_as(C.c_void_p) if use.size else None,
                                     C.byref(n_used), C.byref(n_events)) == 0
    kept = prof(name, False)
    assert n_used.value == len(ref.counted(m)) and n_events.value == int(kept[0].sum() + kept[1].sum()) + kept[2] + kept[3]


def test_one_bin_holds_more_than_a_16_bit_word():
    import mia_amd
    hip = mia_amd.MiaHip(0)
    m = case("prof:prof_one_bin")
    tally(hip, m)
    count, dele, bad, beyond = hip.ma_profile(m.ref_seq)
    assert count[15, 0, 0] == 71680 == count.sum() and dele.sum() == 0 and (bad, beyond) == (0, 0)


def test_records_in_reversed_order_give_the_same_counts():
    import mia_amd
    hip = mia_amd.MiaHip(0)
    for name in ("prof:prof_classes", "prof:prof_edges_%d" % (pc.WG + 1), "prof:prof_tail"):
        m = case(name)
        back = pc.reversed_records(m)
        tally(hip, m)
        a = hip.ma_profile(m.ref_seq, use_of(m))
        tally(hip, back)
        b = hip.ma_profile(back.ref_seq, use_of(back))
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2:] == b[2:], name
        assert np.array_equal(a[0], prof(name, False)[0]), name


def test_jobs_of_other_sizes_and_the_other_exports_through_one_context():
    """large, small, larger, none, small: the buffers grow and are used again; the ACE export, the region view and the SAM export
    before and after"""
    import mia_amd
    hip = mia_amd.MiaHip(0)
    for name in ("sam:sam_4097", "prof:prof_edges_65", "ace:column300", "prof:prof_empty", "prof:prof_edges_17"):
        m = case(name)
        tally(hip, m)
        before = hip.ma_ace() + hip.ma_region(0, m.L - 1) + hip.ma_sam(m.ref_seq)
        hip.stage_stats(reset=True)
        check_profile(hip, m, name, prof(name, False), prof(name, True))
        check_profile(hip, m, name + " (again)", prof(name, False), prof(name, True))
        st = hip.stage_stats(reset=True)
        assert st["k_ma_profile"][1] == (4 if m.rec else 0)
        after = hip.ma_ace() + hip.ma_region(0, m.L - 1) + hip.ma_sam(m.ref_seq)
        assert len(before) == len(after) and all(np.array_equal(a, b) for a, b in zip(before, after)), name
        print("%s: %d records, %d columns; k_ma_profile %.3f ms (four calls)" % (name, len(m.rec), sum(r["end"] - r["start"] + 1 for r in m.rec), st["k_ma_profile"][0]))


def test_call_order_and_refusal():
    import mia_amd
    hip = mia_amd.MiaHip(0)
    n, e = C.c_int64(), C.c_int64()
    good = case("prof:prof_tail")
    seq = C.c_char_p(good.ref_seq.encode("latin1"))
    assert hip._l.mia_hip_ma_profile(hip._h, seq, None, C.byref(n), C.byref(e)) == ERR_STATE             # no tally yet
    assert hip._l.mia_hip_get_ma_profile(hip._h, None, None, None, None) == ERR_STATE
    tally(hip, good)
    assert hip._l.mia_hip_get_ma_profile(hip._h, None, None, None, None) == ERR_STATE                    # tallied, no profile
    assert hip._l.mia_hip_ma_profile(hip._h, None, None, C.byref(n), C.byref(e)) == ERR_ARG              # no reference
    assert hip._l.mia_hip_get_ma_profile(hip._h, None, None, None, None) == ERR_STATE
    check_profile(hip, good, "prof_tail after a refusal", prof("prof:prof_tail", False), prof("prof:prof_tail", True))
    assert hip._l.mia_hip_ma_profile(hip._h, seq, None, None, None) == 0                                  # the two counts may be NULL
    assert hip._l.mia_hip_get_ma_profile(hip._h, None, None, None, None) == 0                             # every pointer of the getter may be NULL
    with pytest.raises(Exception):                                                                        # a bad code on a base: the tally refuses
        tally(hip, pc.bad_on_base())
    assert hip._l.mia_hip_ma_profile(hip._h, seq, None, C.byref(n), C.byref(e)) == ERR_STATE             # and leaves no records behind
    other = case("prof:prof_classes")
    tally(hip, other)
    assert hip._l.mia_hip_get_ma_profile(hip._h, None, None, None, None) == ERR_STATE                    # a new tally: no profile yet
    check_profile(hip, other, "prof_classes after the refusals", prof("prof:prof_classes", False), prof("prof:prof_classes", True))
