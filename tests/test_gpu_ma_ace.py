"""ma_hip's ACE export (-f 7) and rewrite (-m) must be, byte for byte, what the reference's own `ma` prints and writes (the file from its
second line on: the first carries the date), for every run recorded in tests/golden/ma_ace (tools/make_ma_ace_goldens.py, from
oracle/_ref/ma; outputs above 200 000 bytes pinned by sha256) -- and the library call behind the export (mia_hip_ma_ace: layout and one
wavefront per record on the device) must give, per record, what tests/ma_ace_ref.py says, which tests/test_ma_ace_cpu.py holds against
the same recordings."""
import copy
import ctypes as C
import gzip
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import ma_ace_ref as ref
import maln_ace_cases as mc
import maln_synth as ms
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

MA = os.path.join(ROOT, "mapping-iterative-assembler_amd", "ma_hip")
ACE = os.path.join(GOLDEN, "ma_ace")
ERR_ARG, ERR_STATE = -2, -4                # MIA_HIP_ERR_ARG, MIA_HIP_ERR_STATE (include/mia_hip.h)


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(ACE, "hashes.json")) as f:
        hashes = json.load(f)
    with gzip.open(os.path.join(ACE, "outputs.json.gz")) as f:
        outputs = json.load(f)
    return hashes, outputs


@pytest.fixture(scope="module")
def cases():
    return {name: mc.make_case(name) for name in ("shapes", "column300", "empty", "scan16_4096", "fix_lin.1", "fix_c.1") + mc.SCAN_EDGES}


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("ma_ace")
    paths = {}
    for name in mc.CASES + mc.REFUSED:
        paths[name] = str(d / (name + ".maln"))
        with open(paths[name], "w", encoding="latin1") as f:
            f.write(ms.MA_HEADER + mc.case_text(name))
    return paths


def ma_hip(path, args, out=None):
    return subprocess.run([MA, "-M", path] + [out if a == "OUT" else a for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


def same(recorded, name, key, what, raw):
    hashes, outputs = recorded
    h = hashes[f"{name}.{key}.{what}"]
    full = outputs[name][key].get(what)
    if full is not None and raw != full.encode("latin1"):
        a, b = raw.split(b"\n"), full.encode("latin1").split(b"\n")
        at = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        pytest.fail(f"{name} {key} {what}: line {at + 1}: {a[at:at + 1]!r} instead of {b[at:at + 1]!r}")
    assert (len(raw), hashlib.sha256(raw).hexdigest()) == (h["bytes"], h["sha256"]), (name, key, what)


def written(path):
    with open(path, "rb") as f:
        return f.read().split(b"\n", 1)[1]


@pytest.mark.parametrize("name", mc.CASES)
def test_ace_and_rewrite_identical(recorded, files, name, tmp_path):
    for key, args in mc.RUNS.items():
        out = str(tmp_path / (key + ".maln"))
        r = ma_hip(files[name], args, out)
        assert r.returncode == 0, (key, r.stderr[-300:])
        same(recorded, name, key, "stdout", r.stdout)        # f7*: the ACE text; m: the default report; mc2I: the -f 5 sequence
        if "OUT" in args:
            same(recorded, name, key, "file", written(out))


def test_ace_and_rewrite_in_one_run(recorded, files, tmp_path):
    for name in ("shapes", "fix_c.2"):
        out = str(tmp_path / (name + ".maln"))
        r = ma_hip(files[name], ["-f", "7", "-m", out])
        assert r.returncode == 0, r.stderr[-300:]
        same(recorded, name, "f7c1", "stdout", r.stdout)
        same(recorded, name, "m", "file", written(out))


def test_file_without_an_ace_export_is_refused_by_ma_hip(files):
    r = ma_hip(files["gaps0"], ["-f", "7"])
    assert r.returncode == 1 and r.stdout == b""
    assert len(r.stderr.strip().split(b"\n")) == 1 and b"outside the MI355X-accelerated path" not in r.stderr
    r = ma_hip(files["gaps0"], ["-f", "3"])
    assert r.returncode != 0 and b"outside the MI355X-accelerated path" in r.stderr


# ---- the library call ------------------------------------------------------------------------------------------------------------
def sorted_maln(m):
    s = copy.copy(m)
    s.rec = ref.sorted_records(m)
    return s


def tally(hip, m):
    hip.set_pssm(m.fpsm, m.rpsm)
    hip.ma_tally(*ms.ma_tally_args(ms.flatten(sorted_maln(m))))


def check_ace(hip, m, name):
    af, plen, off, body = hip.ma_ace()
    want = ref.layout(m)
    recs = ref.sorted_records(m)
    assert len(af) == len(plen) == len(want) and len(off) == len(want) + 1 and off[0] == 0 and off[-1] == len(body), name
    at = 0
    for i, (w_af, w_len, w_text) in enumerate(want):
        rid = recs[i]["id"]
        assert (int(af[i]), int(plen[i]), int(off[i])) == (w_af, w_len, at), f"{name}: record {i} ({rid}): af_pos, padded_len, body_off"
        w = np.frombuffer(ref.lines50(w_text).encode("latin1"), np.uint8)
        got = body[at:at + len(w)]
        if not np.array_equal(got, w):
            c = int(np.flatnonzero(got != w)[0]) if len(got) == len(w) else min(len(got), len(w))
            pytest.fail(f"{name}: record {i} ({rid}): byte {c} of its text is {bytes(got[c:c + 1])!r}, not {bytes(w[c:c + 1])!r}")
        at += len(w)
    assert at == len(body), name


@pytest.mark.parametrize("name", ["shapes", "fix_c.1", "empty"] + list(mc.SCAN_EDGES))
def test_library_call_matches_the_restatement(cases, name):
    import mia_amd
    hip = mia_amd.MiaHip(0)
    tally(hip, cases[name])
    hip.stage_stats(reset=True)
    check_ace(hip, cases[name], name)
    st = hip.stage_stats()
    n = len(cases[name].rec)
    assert st["k_ma_ace_layout"][1] == (1 if n else 0) and st["k_ma_ace_render"][1] == (1 if n else 0)


def test_three_jobs_and_the_region_view_through_one_context(cases):
    """large, small, large: the buffers grow and are used again; the region view before and after the export"""
    import mia_amd
    hip = mia_amd.MiaHip(0)
    for name in ("column300", "fix_lin.1", "scan16_4096"):
        m = cases[name]
        tally(hip, m)
        rows_a, text_a = hip.ma_region(0, m.L - 1)
        check_ace(hip, m, name)
        rows_b, text_b = hip.ma_region(0, m.L - 1)
        check_ace(hip, m, name + " (again)")
        assert len(rows_a) == len(m.rec) and np.array_equal(rows_a, rows_b) and np.array_equal(text_a, text_b), name
        st = hip.stage_stats(reset=True)
        print("%s: %d records, %d bytes; k_ma_ace_layout %.3f ms, k_ma_ace_render %.3f ms (two calls each)" %
              (name, len(m.rec), sum(len(t) + len(t) // 50 + 1 for _, _, t in ref.layout(m)), st["k_ma_ace_layout"][0], st["k_ma_ace_render"][0]))


def test_call_order_and_refusal(cases):
    import mia_amd
    hip = mia_amd.MiaHip(0)
    n, b = C.c_int64(), C.c_int64()
    assert hip._l.mia_hip_ma_ace(hip._h, C.byref(n), C.byref(b)) == ERR_STATE          # no tally yet
    assert hip._l.mia_hip_get_ma_ace(hip._h, None, None, None, None, 0) == ERR_STATE
    bad = mc.make_case("gaps0")
    tally(hip, bad)
    assert hip._l.mia_hip_ma_ace(hip._h, C.byref(n), C.byref(b)) == ERR_ARG
    assert hip._l.mia_hip_get_ma_ace(hip._h, None, None, None, None, 0) == ERR_STATE
    rows, _ = hip.ma_region(0, bad.L - 1)                                                # the refused job still has its region view
    assert len(rows) == len(bad.rec)
    neg = copy.copy(cases["fix_lin.1"])
    neg.gaps = neg.gaps.copy()
    neg.gaps[neg.L // 2] = -1
    tally(hip, neg)
    assert hip._l.mia_hip_ma_ace(hip._h, C.byref(n), C.byref(b)) == ERR_ARG
    tally(hip, cases["shapes"])
    check_ace(hip, cases["shapes"], "shapes after two refusals")
