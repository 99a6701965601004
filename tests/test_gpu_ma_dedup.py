"""The duplicate filter on the GPU: MiaHip.ma_dedup (mia_hip_ma_dedup: keys, a radix sort, runs, next, pointer doubling, clusters --
csrc/mia_ma_dedup_kernels.h) must give exactly keep, rep, the size histogram and the totals of tests/ma_dedup_ref.py, the rule of
DESIGN.md ("Duplicate filter") restated as a sort and a serial walk, for every shape of tests/maln_dedup_cases.py and every tolerance;
and ma_hip -u [-t N] must print, byte for byte, what ma_hip prints without -u for the file the restatement has already reduced."""
import ctypes as C
import gzip
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import ma_dedup_ref as ref
import maln_dedup_cases as dc
import maln_synth as ms
from conftest import ROOT

pytestmark = pytest.mark.gpu

MA = os.path.join(ROOT, "mapping-iterative-assembler_amd", "ma_hip")
ERR_ARG, ERR_STATE = -2, -4                # MIA_HIP_ERR_ARG, MIA_HIP_ERR_STATE (include/mia_hip.h)
_want = {}


def want(name, t):
    if (name, t) not in _want:
        m = dc.case(name)
        _want[name, t] = ref.dedup(m.rec, m.L, t)
    return _want[name, t]


@pytest.fixture(scope="module")
def hip():
    import mia_amd
    return mia_amd.MiaHip(0)


def check(got, wanted, what):
    keep, rep, hist, n_mol, n_clu, orphans = got
    assert (n_mol, n_clu, orphans) == wanted[3:], what
    assert np.array_equal(hist, wanted[2]), what
    bad = np.nonzero(keep != wanted[0])[0]
    assert bad.size == 0, (what, "keep", bad[:5].tolist())
    bad = np.nonzero(rep != wanted[1])[0]
    assert bad.size == 0, (what, "rep", bad[:5].tolist(), rep[bad[:5]].tolist(), wanted[1][bad[:5]].tolist())


def write(m, path):
    with open(path, "w", encoding="latin1") as f:
        f.write(ms.MA_HEADER + ms.write_maln(m))
    return path


def ma_hip(path, args):
    return subprocess.run([MA, "-M", path] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


@pytest.mark.parametrize("name", dc.CASES + dc.LIBRARY_ONLY)
def test_library_call_matches_the_restatement(hip, name):
    m = dc.case(name)
    start, end, rc, score, mate = ref.device_arrays(m.rec)
    for t in dc.TOLERANCES:
        check(hip.ma_dedup(m.L, start, end, rc, score, mate, t), want(name, t), "%s t=%d" % (name, t))
    if not (mate != -1).any():                               # no halves: mate may be left out
        check(hip.ma_dedup(m.L, start, end, rc, score, None, 2), want(name, 2), name + " without mate")


def test_twice_on_one_context(hip):
    """buffers are reused: large, small, empty, large again"""
    for name, t in (("mixed_20000", 2), ("hand", 1), ("empty", 0), ("pile_5000", 0), ("wrap", 7), ("mixed_20000", 0)):
        m = dc.case(name)
        check(hip.ma_dedup(m.L, *ref.device_arrays(m.rec), t), want(name, t), "%s t=%d in a row" % (name, t))


def test_argument_and_state_errors():
    import mia_amd
    hip = mia_amd.MiaHip(0)
    n1, n2 = C.c_int64(), C.c_int64()
    assert hip._l.mia_hip_get_ma_dedup(hip._h, None, None, None, None) == ERR_STATE                  # no call yet
    m = dc.case("wrap")
    start, end, rc, score, mate = ref.device_arrays(m.rec)

    def call(start=start, end=end, mate=mate, t=0, L=m.L):
        s, e, mt = (np.ascontiguousarray(x) for x in (start, end, mate))
        return hip._l.mia_hip_ma_dedup(hip._h, L, len(s), s.ctypes.data_as(C.c_void_p), e.ctypes.data_as(C.c_void_p), rc.ctypes.data_as(C.c_void_p),
                                       score.ctypes.data_as(C.c_void_p), mt.ctypes.data_as(C.c_void_p), t, C.byref(n1), C.byref(n2))

    def changed(a, i, v):
        b = a.copy()
        b[i] = v
        return b

    pair = int(np.nonzero(mate >= 0)[0][0])
    whole = int(np.nonzero(mate == -1)[0][0])
    for what, code in (("t=-1", call(t=-1)), ("t=101", call(t=101)), ("start<0", call(start=changed(start, whole, -1))),
                       ("end<start-1", call(end=changed(end, whole, start[whole] - 2))), ("end>=2L", call(end=changed(end, whole, 2 * m.L))),
                       ("mate out of range", call(mate=changed(mate, whole, len(mate)))), ("mate below -2", call(mate=changed(mate, whole, -3))),
                       ("mate is itself", call(mate=changed(mate, whole, whole))), ("mate not mutual", call(mate=changed(mate, whole, pair))),
                       ("L=0", call(L=0))):
        assert code == ERR_ARG, what
        assert hip._l.mia_hip_get_ma_dedup(hip._h, None, None, None, None) == ERR_STATE, what            # a refused call leaves no result
    assert call(end=changed(end, whole, start[whole] - 1)) == 0                                          # a record without columns is valid
    assert call(t=100) == 0
    check(hip.ma_dedup(m.L, start, end, rc, score, mate, 7), want("wrap", 7), "wrap after the refusals")
    assert hip._l.mia_hip_get_ma_dedup(hip._h, None, None, None, None) == 0                              # every pointer may be NULL


FORMATS = {"f41": ["-f", "41", "-c", "1"], "f5": ["-f", "5"], "f42A": ["-f", "42", "-A"], "f8m": ["-f", "8", "-m", None], "f93": ["-f", "93"]}


GOLD = os.path.join(ROOT, "tests", "golden", "ma_dedup")
GOLD_TAG = {"f41": "f41c1", "f5": "f5"}
_gold = []


def reference_cases():
    """tests/golden/ma_dedup/outputs.json.gz (tools/make_ma_dedup_goldens.py), "cases": the reference's ma on the files the restatement
    reduced; "sets": its ma on its own `mia -u` runs"""
    if not _gold:
        with gzip.open(os.path.join(GOLD, "outputs.json.gz")) as f:
            _gold.append(json.load(f))
    return _gold[0]["cases"]


# every format on four cases; the formats the reference has a golden for on the shapes that stress the anchors' walk
END_TO_END = [(name, t, fmt) for name, t in (("hand", 0), ("hand", 2), ("wrap", 0), ("wrap", 2), ("ins_only_in_dups", 0), ("mixed_20000", 0),
                                             ("mixed_20000", 2)) for fmt in sorted(FORMATS)] + \
    [(name, 2, fmt) for name in ("stairs_4097", "stairs_rev", "e_ladder", "strand_seam", "runs_edge") for fmt in ("f41", "f5")]


@pytest.mark.parametrize("name,t,fmt", END_TO_END)
def test_ma_hip_u_is_ma_hip_on_the_reduced_file(name, t, fmt, tmp_path):
    m = dc.case(name)
    full = write(m, str(tmp_path / "full.maln"))
    less = write(ref.reduce(m, want(name, t)[0]), str(tmp_path / "less.maln"))
    outs = []
    for path, extra, tag in ((full, ["-u"] + (["-t", str(t)] if t else []), "u"), (less, [], "plain")):
        out = str(tmp_path / (tag + ".maln"))
        args = [out if a is None else a for a in FORMATS[fmt]]
        r = ma_hip(path, args + extra)
        assert r.returncode == 0, (args, r.stderr[-300:])
        body = open(out, "rb").read().split(b"\n", 1)[1] if None in FORMATS[fmt] else b""
        outs.append((r.stdout, body))
    assert outs[0][0] == outs[1][0], (name, t, fmt)
    assert outs[0][1] == outs[1][1], (name, t, fmt, "-m")
    if None in FORMATS[fmt]:
        assert outs[0][1].startswith(b"MALN_NAS %d\n" % int(want(name, t)[0].sum()))
    if fmt in GOLD_TAG:                                      # ... and what the compiled reference's ma printed for the reduced file
        gold = reference_cases()[name][str(t)][GOLD_TAG[fmt]]
        if isinstance(gold, dict):
            assert (len(outs[0][0]), hashlib.sha256(outs[0][0]).hexdigest()) == (gold["bytes"], gold["sha256"]), (name, t, fmt)
        else:
            assert outs[0][0] == gold.encode("latin1"), (name, t, fmt)


@pytest.mark.parametrize("tag,args", (("f41c1", ["-f", "41", "-c", "1"]), ("f5c1", ["-f", "5", "-c", "1"]), ("f5c2", ["-f", "5", "-c", "2"])))
@pytest.mark.parametrize("name", dc.READ_SETS)
def test_ma_hip_u_on_the_references_run_is_the_references_ma_on_its_u_run(name, tag, args, tmp_path):
    """<set>.maln.1.gz is the compiled reference's `mia -c -n -H 1` on a read set, without -u; outputs.json.gz holds its own `ma` on its
    own `mia -c -n -H 1 -u` run of the same reads: parse, pairing by ID, the device's filter, removal and GAPS, end to end"""
    path = str(tmp_path / "in.maln")
    with gzip.open(os.path.join(GOLD, name + ".maln.1.gz"), "rb") as f, open(path, "wb") as g:
        g.write(f.read())
    r = ma_hip(path, ["-u"] + args)
    assert r.returncode == 0, r.stderr[-300:]
    reference_cases()
    assert r.stdout == _gold[0]["sets"][name][tag].encode("latin1"), (name, tag)


def test_halves_that_do_not_lie_across_the_origin_are_refused_with_a_message(tmp_path):
    """the device takes the half with the greater START as the front, so ma_hip -u refuses a file whose _f half does not start behind
    its _b half (no mia writes one); without -u the file is read as ever"""
    m = dc.make_case("strand_seam")
    dc._add(m, "odd_f", 10, 30, seg="f", score=5)
    dc._add(m, "odd_b", 40, 60, seg="b", score=5)
    path = write(m, str(tmp_path / "in.maln"))
    r = ma_hip(path, ["-u", "-f", "41"])
    assert r.returncode != 0 and b"odd_" in r.stderr and b"origin" in r.stderr and r.stdout == b""
    assert ma_hip(path, ["-f", "41"]).returncode == 0


def test_gaps_line_of_the_filtered_file(tmp_path):
    for name, fmt, left in (("ins_only_in_dups", "5", ["alone", "alone_rev", "best"]), ("ins_repeat", "5", ["kept"])):
        m = dc.case(name)
        out = str(tmp_path / "out.maln")
        r = ma_hip(write(m, str(tmp_path / "in.maln")), ["-u", "-f", fmt, "-m", out])
        assert r.returncode == 0, r.stderr[-300:]
        got = ms.parse_maln(open(out, encoding="latin1").read().split("\n", 1)[1])
        assert np.array_equal(got.gaps, ref.new_gaps(m, want(name, 0)[0])), name
        assert not np.array_equal(got.gaps, m.gaps) and sorted(x["id"] for x in got.rec) == left


def test_t_needs_u_and_a_value_in_range(tmp_path):
    path = write(dc.case("hand"), str(tmp_path / "in.maln"))
    r = ma_hip(path, ["-f", "41", "-t", "2"])
    assert r.returncode != 0 and b"-t" in r.stderr and b"-u" in r.stderr and r.stdout == b""
    for bad in ("101", "-1", "x", "2.5"):
        r = ma_hip(path, ["-u", "-t", bad])
        assert r.returncode != 0 and b"-t" in r.stderr and r.stdout == b"", bad
    r = subprocess.run([MA], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert b"-u" in r.stdout and b"-t" in r.stdout
