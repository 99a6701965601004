"""k_ma_tally, k_ma_ins_events, k_ins_tally, the insert calls, the insert-offset prefix sum and the string assembly on the synthetic
.maln cases of tests/maln_synth.py: deep columns, insert slots thousands of records deep on both strands, insert columns on the
block and stretch edges, every depth code, jobs of different sizes through one context.

Truth is the reference's own `ma`: its recorded output (tests/golden/ma_synth, tools/make_ma_synth_goldens.py) for ma_hip's bytes,
and for the library the numpy restatement that tests/test_ma_synth_cpu.py holds against that output line by line -- so a mismatch
here names a column, a slot and a word.  Nothing is compared with the HIP path itself, nothing is sampled."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import maln_synth as ms
from conftest import ROOT
from test_ma_synth_cpu import case, initial_insert_capacity, recorded

pytestmark = pytest.mark.gpu

MA = os.path.join(ROOT, "mapping-iterative-assembler_amd", "ma_hip")
NAMES = list(ms.CASES)
T_SPAN = 10
_flat = {}


def flat(name):
    if name not in _flat:
        _flat[name] = ms.flatten(case(name)[0])
    return _flat[name]


@pytest.mark.parametrize("name", NAMES)
def test_ma_hip_prints_what_the_reference_printed(name, tmp_path):
    m, r = case(name)
    path = str(tmp_path / (name + ".maln"))
    with open(path, "w", encoding="latin1") as f:
        f.write(ms.MA_HEADER + ms.write_maln(m))
    for key in ms.RUN_KEYS + ("f4c2",):
        fmt, code = key[1:].split("c")
        out = subprocess.run([MA, "-M", path, "-f", fmt, "-c", code], check=True, stdout=subprocess.PIPE, timeout=120).stdout
        if key in ms.RUN_KEYS:
            want, h = recorded(name, key)
        else:                                   # -f 4 -c 2 is not among the recorded runs: the restatement stands in, whose -f 4 -c 1
            want, h = r.output(key), None       # and -f 41 -c 2 the CPU test holds against the reference
        if want is not None and out != want.encode("latin1"):
            a, b = out.decode("latin1").split("\n"), want.split("\n")
            k = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            pytest.fail(f"{name} {key}: line {k}: ma_hip {a[k:k + 1]} reference {b[k:k + 1]}")
        if h is not None:
            assert (len(out), hashlib.sha256(out).hexdigest()) == (h["bytes"], h["sha256"]), (name, key)


def first_difference(got, want, names, what):
    """None, or the first (row, word) at which two [rows][words] arrays differ, with both values"""
    if got.shape != want.shape:
        return f"{what}: shape {got.shape}, expected {want.shape}"
    bad = np.argwhere(got != want)
    if len(bad) == 0:
        return None
    i, w = bad[0]
    return f"{what} {i}, word {names[w]}: GPU {got[i, w]}, reference {want[i, w]} ({len(bad)} words differ)"


def run_and_compare(hip, name):
    """one job through MiaHip: every word of every column and insert slot, the offsets and both strings"""
    m, r = case(name)
    L = m.L
    hip.set_pssm(m.fpsm, m.rpsm)
    hip.ma_tally(*ms.ma_tally_args(flat(name)))
    tally, gaps = hip.get_tally()
    assert tally.shape == (12, L + 1)
    assert (gaps[:L] == m.gaps).all() and gaps[L] == 0
    where = f"{name}: "
    diff = first_difference(tally[:10, :L].T.astype(np.int64), r.cols.T, ms.COL_WORDS, "column")
    assert diff is None, where + diff
    diff = first_difference(tally[T_SPAN:T_SPAN + 1, :L].T.astype(np.int64), r.span[:, None], ("T_SPAN",), "column")
    assert diff is None, where + diff
    assert not tally[:11, L].any(), where + "the padding column behind the reference was written"
    for code in (1, 2):
        got = hip.consensus(code)
        off, ins = hip.ins_tally()
        diff = first_difference(off[:, None].astype(np.int64), r.ins_off[:, None], ("ins_off",), "column")
        assert diff is None, where + diff
        diff = first_difference(ins.astype(np.int64), r.ins, ms.INS_WORDS, "insert slot")
        if diff is not None:
            s = int(diff.split()[2].rstrip(","))
            pytest.fail(where + diff + f" (column {r.slot_col[s]}, gap position {s - r.ins_off[r.slot_col[s]]}, consensus code {code})")
        want = r.consensus(code)
        if got != want:
            k = next((i for i, (x, y) in enumerate(zip(got, want)) if x != y), min(len(got), len(want)))
            pytest.fail(where + f"consensus code {code}: lengths {len(got)} / {len(want)}, first difference at character {k}: GPU {got[k:k + 20]!r}, reference {want[k:k + 20]!r}")


@pytest.fixture(scope="module")
def shared_hip():
    import mia_amd
    hip = mia_amd.MiaHip(0)
    yield hip
    hip.close()


@pytest.mark.parametrize("name", NAMES)
def test_library_matches_the_reference_word_for_word(name, shared_hip):
    """(one context for all the cases, in the order of CASES: three columns first, twenty thousand records in the middle)"""
    run_and_compare(shared_hip, name)


def test_three_jobs_through_one_context():
    """deep, edge256, deep: stale column tallies, stale insert tallies, the event list and the insert buffers sized by another job"""
    import mia_amd
    assert len(case("deep")[1].ins) > initial_insert_capacity() and len(case("deep")[1].ins) > len(case("edge256")[1].ins)
    hip = mia_amd.MiaHip(0)
    try:
        for name in ("deep", "edge256", "deep"):
            run_and_compare(hip, name)
    finally:
        hip.close()


BAD = {
    # a record of three columns from L - 1 on: columns L - 1, L and L + 1 (the tally has one padding column, L)
    "past_the_reference": lambda L: dict(start=[L - 1], seq=b"ACG", smp=b"ABC"),
    "code_above": lambda L: dict(start=[0], seq=b"ACG", smp=b"A`C"),
    "code_below": lambda L: dict(start=[0], seq=b"ACG", smp=b"A@C"),
}


@pytest.mark.parametrize("what", list(BAD))
def test_rejected_input_leaves_the_context_usable(what):
    import mia_amd
    m, _ = case("edge256")
    bad = BAD[what](m.L)
    hip = mia_amd.MiaHip(0)
    try:
        hip.set_pssm(m.fpsm, m.rpsm)
        with pytest.raises(mia_amd.MiaHipError):
            hip.ma_tally(m.L, m.gaps, bad["start"], [0], [0, 3], bad["seq"], bad["smp"])
        run_and_compare(hip, "edge256")
        # a depth code outside A.._ under a '-' is never looked at (add_base returns first, src/map_align.c:251-253)
        hip.ma_tally(m.L, m.gaps, [0], [0], [0, 3], b"A-G", b"A`C")
        tally, _ = hip.get_tally()
        assert tally[4, 1] == 1 and tally[5, :3].tolist() == [1, 1, 1]
        run_and_compare(hip, "edge256")
    finally:
        hip.close()
