"""ma_hip's SAM export (-f 8).  The reference's `ma` has no SAM output, so nothing recorded from it pins this report: ma_hip must
print, byte for byte, the header and the lines of tests/ma_sam_ref.py (the rule of DESIGN.md restated in Python, which
tests/test_ma_sam_cpu.py holds to the way back from every line to its record), and the library call behind it (mia_hip_ma_sam: layout
and one wavefront per record on the device) must give NM, offset and body per record.  The shapes at which the kernels can go wrong
are those of tests/maln_sam_cases.py."""
import copy
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ma_ace_ref as ace_ref
import ma_sam_ref as ref
import maln_ace_cases as mc
import maln_sam_cases as sc
import maln_synth as ms
from conftest import ROOT

pytestmark = pytest.mark.gpu

MA = os.path.join(ROOT, "mapping-iterative-assembler_amd", "ma_hip")
ERR_ARG, ERR_STATE = -2, -4                # MIA_HIP_ERR_ARG, MIA_HIP_ERR_STATE (include/mia_hip.h)
# the ACE cases (three of them committed .maln), the ten cases of maln_synth (GAPS[0] = 3: fine here), the SAM shapes
NAMES = tuple("ace:" + n for n in mc.CASES) + tuple("synth:" + n for n in ms.CASES) + tuple("sam:" + n for n in sc.CASES)
_made = {}


def case(name):
    if name not in _made:
        kind, key = name.split(":", 1)
        _made[name] = {"ace": mc.make_case, "synth": ms.make_case, "sam": sc.make_case}[kind](key)
    return _made[name]


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
def test_sam_identical(name, tmp_path):
    m = case(name)
    path = write(m, str(tmp_path / "in.maln"))
    for args, new_id in ((["-f", "8"], None), (["-f", "8", "-I", "my_contig"], "my_contig")):
        r = ma_hip(path, args)
        assert r.returncode == 0, (args, r.stderr[-300:])
        same_text("%s %s" % (name, " ".join(args)), r.stdout, ref.sam(m, new_id))


def test_sam_and_rewrite_in_one_run(tmp_path):
    m = case("ace:shapes")
    path, out = write(m, str(tmp_path / "in.maln")), str(tmp_path / "out.maln")
    r = ma_hip(path, ["-f", "8", "-c", "2", "-I", "my_contig", "-m", out])
    assert r.returncode == 0, r.stderr[-300:]
    same_text("shapes -f 8 -m", r.stdout, ref.sam(m, "my_contig"))
    with open(out, "rb") as f:
        same_text("shapes -m file", f.read().split(b"\n", 1)[1], ace_ref.rewrite(m, 2, "my_contig"))


def test_negative_gap_is_refused_by_ma_hip(tmp_path):
    path = write(sc.negative_gap(case("sam:sam_257")), str(tmp_path / "neg.maln"))
    r = ma_hip(path, ["-f", "8"])
    assert r.returncode == 1 and r.stdout == b"" and len(r.stderr.strip().split(b"\n")) == 1


# ---- the library call ------------------------------------------------------------------------------------------------------------
def sorted_maln(m):
    s = copy.copy(m)
    s.rec = ref.sorted_records(m)
    return s


def tally(hip, m):
    hip.set_pssm(m.fpsm, m.rpsm)
    hip.ma_tally(*ms.ma_tally_args(ms.flatten(sorted_maln(m))))


def wanted(m):
    """per sorted record (id, NM, body)"""
    out = []
    for r in ref.sorted_records(m):
        b, nm = ref.body(r, m.L, m.ref_seq)
        out.append((r["id"], nm, b.encode("latin1")))
    return out


def check_sam(hip, m, name, want=None):
    nm, off, body = hip.ma_sam(m.ref_seq)
    want = wanted(m) if want is None else want
    assert len(nm) == len(want) and len(off) == len(want) + 1 and off[0] == 0 and off[-1] == len(body), name
    at = 0
    raw = body.tobytes()
    for i, (rid, w_nm, w_body) in enumerate(want):
        assert (int(nm[i]), int(off[i])) == (w_nm, at), f"{name}: record {i} ({rid}): NM, body_off"
        got = raw[at:at + len(w_body)]
        if got != w_body:
            c = next((k for k, (x, y) in enumerate(zip(got, w_body)) if x != y), min(len(got), len(w_body)))
            pytest.fail(f"{name}: record {i} ({rid}): byte {c} of its body: {got[max(0, c - 20):c + 10]!r}, not {w_body[max(0, c - 20):c + 10]!r}")
        at += len(w_body)
    assert at == len(body), name


@pytest.mark.parametrize("name", ["sam:sam_shapes", "sam:sam_lower", "sam:sam_257", "sam:sam_4097", "sam:sam_empty", "ace:shapes", "ace:fix_c.1", "synth:edge257"] +
                         ["ace:" + n for n in mc.SCAN_EDGES] + ["sam:" + n for n in sc.SCAN_EDGES])
def test_library_call_matches_the_restatement(name):
    import mia_amd
    hip = mia_amd.MiaHip(0)
    m = case(name)
    tally(hip, m)
    hip.stage_stats(reset=True)
    check_sam(hip, m, name)
    st = hip.stage_stats()
    n = len(m.rec)
    assert st["k_ma_sam_layout"][1] == (1 if n else 0) and st["k_ma_sam_render"][1] == (1 if n else 0)


def test_jobs_of_other_sizes_and_the_other_exports_through_one_context():
    """large, small, larger, none, small: the buffers grow and are used again; the ACE export and the region view before and after"""
    import mia_amd
    hip = mia_amd.MiaHip(0)
    for name in ("ace:column300", "sam:sam_shapes", "ace:scan16_4096", "sam:sam_empty", "sam:sam_257"):
        m = case(name)
        want = wanted(m)
        tally(hip, m)
        ace_a = hip.ma_ace()
        rows_a, text_a = hip.ma_region(0, m.L - 1)
        hip.stage_stats(reset=True)
        check_sam(hip, m, name, want)
        check_sam(hip, m, name + " (again)", want)
        st = hip.stage_stats(reset=True)
        ace_b = hip.ma_ace()
        rows_b, text_b = hip.ma_region(0, m.L - 1)
        assert all(np.array_equal(a, b) for a, b in zip(ace_a, ace_b)) and np.array_equal(rows_a, rows_b) and np.array_equal(text_a, text_b), name
        print("%s: %d records, %d bytes of bodies; k_ma_sam_layout %.3f ms, k_ma_sam_render %.3f ms (two calls each)" %
              (name, len(m.rec), sum(len(b) for _, _, b in want), st["k_ma_sam_layout"][0], st["k_ma_sam_render"][0]))


def test_call_order_and_refusal():
    import mia_amd
    hip = mia_amd.MiaHip(0)
    n, b = C.c_int64(), C.c_int64()
    good = case("sam:sam_257")
    seq = C.c_char_p(good.ref_seq.encode("latin1"))
    assert hip._l.mia_hip_ma_sam(hip._h, seq, C.byref(n), C.byref(b)) == ERR_STATE            # no tally yet
    assert hip._l.mia_hip_get_ma_sam(hip._h, None, None, None, 0) == ERR_STATE
    tally(hip, good)
    assert hip._l.mia_hip_get_ma_sam(hip._h, None, None, None, 0) == ERR_STATE                # tallied, not exported
    assert hip._l.mia_hip_ma_sam(hip._h, None, C.byref(n), C.byref(b)) == ERR_ARG             # no reference
    assert hip._l.mia_hip_get_ma_sam(hip._h, None, None, None, 0) == ERR_STATE
    check_sam(hip, good, "sam_257 after a refusal")
    assert hip._l.mia_hip_get_ma_sam(hip._h, None, None, None, 0) == 0                        # every pointer of the getter may be NULL
    tally(hip, sc.negative_gap(good))
    assert hip._l.mia_hip_ma_sam(hip._h, seq, C.byref(n), C.byref(b)) == ERR_ARG              # a negative gap
    assert hip._l.mia_hip_get_ma_sam(hip._h, None, None, None, 0) == ERR_STATE
    first = mc.make_case("gaps0")                                                             # GAPS[0] > 0: no ACE export, but a SAM export
    tally(hip, first)
    assert hip._l.mia_hip_ma_ace(hip._h, C.byref(n), C.byref(b)) == ERR_ARG
    check_sam(hip, first, "gaps0")
    tally(hip, case("sam:sam_shapes"))
    check_sam(hip, case("sam:sam_shapes"), "sam_shapes after the refusals")
