"""The synthetic .maln cases behind tests/test_gpu_ma_synth.py, checked without a GPU: the writer reproduces the reference's text
format, the generator still makes the files the goldens were recorded from, the numpy restatement of the reference's `ma`
(tests/maln_synth.py) prints what the reference itself printed for every case (tests/golden/ma_synth, written by
tools/make_ma_synth_goldens.py from oracle/_ref/ma), and every case has the properties it was made for."""
import glob
import gzip
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

import maln_synth as ms
from conftest import GOLDEN, ROOT

GS = os.path.join(GOLDEN, "ma_synth")
NAMES = list(ms.CASES)
EDGES, SCANS, CODES = ("edge255", "edge256", "edge257"), ("scan16_4095", "scan16_4096", "scan16_4097"), ("codes_anc", "codes_flat")

_cache = {}


def case(name):
    """(Maln, Restated) of a case, made once"""
    if name not in _cache:
        m = ms.make_case(name)
        _cache[name] = (m, ms.restate(m))
    return _cache[name]


def recorded(name, key):
    """(output of the reference or None if only its digest is kept, {sha256, bytes})"""
    if "outputs" not in _cache:
        _cache["outputs"] = json.load(gzip.open(os.path.join(GS, "outputs.json.gz")))
        _cache["hashes"] = json.load(open(os.path.join(GS, "hashes.json")))
    text = _cache["outputs"].get(name, {}).get(key)
    path = os.path.join(GS, f"{name}.{key}.gz")
    if text is None and os.path.exists(path):
        text = gzip.open(path).read().decode("latin1")
    return text, _cache["hashes"][f"{name}.{key}"]


def malns():
    return sorted(glob.glob(os.path.join(GOLDEN, "maln", "*.[0-9]")))


def test_writer_round_trips_every_committed_maln():
    files = malns()
    assert len(files) == 42
    for path in files:
        text = open(path, encoding="latin1").read()
        assert ms.write_maln(ms.parse_maln(text)) == text, path


def test_goldens_cover_the_cases():
    runs = json.load(open(os.path.join(GS, "runs.json")))
    assert runs["keys"] == list(ms.RUN_KEYS)
    assert sorted(k for k in runs if k != "keys") == sorted(NAMES)
    for name in NAMES:
        assert runs[name]["seed"] == ms.CASES[name]["seed"]
        for key in ms.RUN_KEYS:
            text, h = recorded(name, key)
            assert text is not None or name in ms.BIG_CASES, (name, key)
            if text is not None:
                assert (len(text), hashlib.sha256(text.encode("latin1")).hexdigest()) == (h["bytes"], h["sha256"]), (name, key)


@pytest.mark.parametrize("name", NAMES)
def test_generator_has_not_drifted(name):
    runs = json.load(open(os.path.join(GS, "runs.json")))
    m, _ = case(name)
    assert (len(m.rec), ms.maln_sha256(m)) == (runs[name]["records"], runs[name]["sha256"]), \
        f"the generator drifted: tests/maln_synth.py no longer makes the {name} the goldens were recorded from (no kernel is involved)"
    assert ms.write_maln(ms.parse_maln(ms.write_maln(m))) == ms.write_maln(m)


@pytest.mark.parametrize("name", NAMES)
def test_restatement_prints_what_the_reference_printed(name):
    _, r = case(name)
    for key in ms.RUN_KEYS:
        got = r.output(key)
        want, h = recorded(name, key)
        if want is not None and got != want:
            a, b = got.split("\n"), want.split("\n")
            k = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            pytest.fail(f"{name} {key}: line {k}: restated {a[k:k + 1]} reference {b[k:k + 1]}")
        assert (len(got), hashlib.sha256(got.encode("latin1")).hexdigest()) == (h["bytes"], h["sha256"]), (name, key)


def longest_insert_before(m):
    """GAPS as mia leaves it: per column the longest insert among the records that start before it"""
    g = np.zeros(m.L, np.int64)
    for r in m.rec:
        for p, s in r["ins"]:
            if p > 0:
                g[r["start"] + p] = max(g[r["start"] + p], len(s))
    return g


@pytest.mark.parametrize("name", NAMES)
def test_rules_every_case_keeps(name):
    m, r = case(name)
    assert abs(len(m.rec) - ms.CASES[name]["n"]) <= 4 and m.L == ms.CASES[name]["L"]
    n_ins = 0
    for rec in m.rec:
        assert set(rec["seq"]) <= set("ACGTN-") and len(rec["seq"]) == len(rec["smp"]) == rec["end"] - rec["start"] + 1 <= 256
        assert 0 <= rec["start"] <= rec["end"] < m.L
        for p, s in rec["ins"]:
            assert set(s) <= set("ACGTN") and 1 <= len(s) <= 40 and 0 <= p <= rec["end"] - rec["start"]
            n_ins += 1
    assert m.gaps[0] > 0                                            # column 0: the reference never looks
    assert (m.gaps[1:] == longest_insert_before(m)[1:]).all()
    if m.L > 1:
        assert n_ins > 0 and len(r.ins) == m.gaps[1:].sum() > 0
        seq = "".join(rec["seq"] for rec in m.rec)
        assert "N" in seq and "-" in seq
    if "clusters" in ms.CASES[name]:
        assert (r.cols[5] == 0).any()                               # columns no record covers
    for col in ms.CASES[name].get("ins", {}):
        # an insert column with records that start on it: they are in the column's coverage, not in the insert's
        starts_here = sum(1 for rec in m.rec if rec["start"] == col)
        spans = sum(1 for rec in m.rec if rec["start"] < col <= rec["end"])
        assert m.gaps[col] == len(ms.CASES[name]["ins"][col]) and starts_here >= 3
        assert r.span[col] == spans and r.cols[5][col] == spans + starts_here
        assert sum(1 for rec in m.rec if rec["end"] == col) >= 3


def test_one_col():
    m, r = case("one_col")
    assert m.L == 1 < 64 and len(m.rec) == 3 and len(r.ins) == 0 and r.cols[5][0] == 3 and len(r.consensus(1)) <= 1


@pytest.mark.parametrize("name", EDGES)
def test_edge_cases_have_inserts_at_the_block_edge(name):
    m, r = case(name)
    want = [1, m.L - 1] + [c for c in (254, 255, 256, 257) if c < m.L]
    for col in want:
        assert m.gaps[col] > 0 and r.ins[r.ins_off[col], 4] > 0, col
    assert any(p == 0 for rec in m.rec for p, _ in rec["ins"])     # an insert in front of a record's own first column
    assert any(c in "ACGT" for c in r.calls(1)[1])                   # and insert calls that reach the string


@pytest.mark.parametrize("name", SCANS)
def test_scan_cases_sit_on_the_stretch_step(name):
    m, r = case(name)

    def stretch(n):                                                   # k_excl_scan: elements per wavefront
        return ((n + 15) // 16 + 255) & ~255

    assert (stretch(4095 + 1), stretch(4096 + 1), stretch(4097 + 1)) == (256, 512, 512)      # the scan runs over L + 1 elements
    for col in [c for c in (1023, 1024, 4095, 4096) if c < m.L] + [m.L - 1]:
        assert m.gaps[col] > 0 and r.ins[r.ins_off[col], 4] > 0, col
        assert find_call(r, r.ins_off[col], 1) in "ACGT"
    if name == "scan16_4096":
        assert m.gaps[1024] == 40


def find_call(r, slot, code):
    return ms.find_consensus(*r.slot_counts(int(slot)), code)[0]


def initial_insert_capacity():
    src = open(os.path.join(ROOT, "mapping-iterative-assembler_amd", "csrc", "mia_hip.hip")).read()
    return int(re.search(r"int64_t ins_tally_cap = (\d+);", src).group(1))


def test_deep():
    m, r = case("deep")
    assert len(m.rec) > 16000                                        # INIT_NUM_ALN_SEQS: the reference grew its array (MALN_SIZ)
    assert m.siz >= len(m.rec)
    assert r.cols[5].max() >= 5000
    ncols = np.array([rec["end"] - rec["start"] + 1 for rec in m.rec])
    assert ncols.min() >= 2 and (ncols >= 30).mean() > 0.99 and ncols.max() == 256
    assert 1_500_000 <= ncols.sum() <= 3_000_000
    assert 0.45 < np.mean([rec["rc"] for rec in m.rec]) < 0.55
    assert len({tuple(m.fpsm[d].ravel()) for d in range(31)}) > 1     # a position-specific matrix
    assert len(r.ins) > initial_insert_capacity()                    # the first consensus call has to enlarge the insert buffers
    deep_cols = [c for c in ms.DEEP_INS if 1 <= m.gaps[c] <= 12 and r.ins[r.ins_off[c], 4] >= 2000]
    assert len(deep_cols) >= 5
    slots = [int(r.ins_off[c]) + j for c in deep_cols for j in range(int(m.gaps[c]))]
    t = {s: r.slot_counts(s) for s in slots}                         # A C G T gaps cov sA sC sG sT
    both = {s for s in slots if all(sum(1 for rec in m.rec if rec["rc"] == strand and rec["start"] < r.slot_col[s] <= rec["end"]) > 1000 for strand in (0, 1))}
    assert both == set(slots)
    # the packed (scoreC << 32) + scoreA sum: a negative low half under a non-negative high half, and the other way round
    assert any(t[s][6] < 0 <= t[s][7] and r.ins[s, 4] >= 2000 for s in slots)
    assert any(t[s][7] < 0 <= t[s][6] and r.ins[s, 4] >= 2000 for s in slots)
    assert any(t[s][8] < 0 <= t[s][9] for s in slots) and any(t[s][9] < 0 <= t[s][8] for s in slots)
    # exactly half gaps calls '-', one gap fewer calls a base
    assert any(2 * t[s][4] == t[s][5] and find_call(r, s, 1) == "-" for s in slots)
    assert any(2 * t[s][4] == t[s][5] - 2 and find_call(r, s, 1) in "ACGT" for s in slots)
    assert any(2 * t[s][4] > t[s][5] and find_call(r, s, 1) == "-" for s in slots)
    assert any(find_call(r, s, 1) == "N" and find_call(r, s, 2) in "ACGT" for s in slots)


@pytest.mark.parametrize("name", CODES)
def test_codes_cases_use_every_depth_code_on_both_strands(name):
    m, _ = case(name)
    seen = {(rec["rc"], c) for rec in m.rec for b, c in zip(rec["seq"], rec["smp"]) if b != "-"}
    assert seen == {(s, chr(ord("A") + d)) for s in (0, 1) for d in range(31)}
    seen_ins = {(rec["rc"], rec["smp"][p]) for rec in m.rec for p, _ in rec["ins"] if p > 0}
    assert {s for s, _ in seen_ins} == {0, 1} and len({c for _, c in seen_ins}) > 15
    lens = {rec["end"] - rec["start"] + 1 for rec in m.rec}
    assert 1 in lens and 256 in lens
    assert (name == "codes_flat") == (len({tuple(m.fpsm[d].ravel()) for d in range(31)}) == 1)


def test_reference_binary_agrees_when_present(tmp_path):
    """one case through the reference afresh, where it was built (oracle/_ref/ma)"""
    ref = os.path.join(ROOT, "oracle", "_ref", "ma")
    m, r = case("edge256")
    if os.path.exists(ref):
        path = str(tmp_path / "edge256.maln")
        with open(path, "w", encoding="latin1") as f:
            f.write(ms.MA_HEADER + ms.write_maln(m))
        for key in ms.RUN_KEYS:
            fmt, code = key[1:].split("c")
            out = subprocess.run([ref, "-M", path, "-f", fmt, "-c", code], check=True, stdout=subprocess.PIPE, timeout=60).stdout.decode("latin1")
            assert out == recorded("edge256", key)[0] == r.output(key), key
