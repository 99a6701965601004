"""ma_hip's clustalw and line reports (-f 1, the default, and -f 2) and its region view (-f 6 / -f 61 with -R, -C, -I) must be,
byte for byte, what the reference's own `ma` prints, for every run recorded in tests/golden/ma_region (written by
tools/make_ma_region_goldens.py from oracle/_ref/ma; outputs above 40 KB pinned by sha256) -- and the library call behind the
region view (mia_hip_ma_region: ordered selection and one row per selected record on the device) must give, on a million
synthetic records, what the row rule says when it is written down in numpy."""
import gzip
import hashlib
import json
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import maln_ace_cases as mc
import maln_synth as ms
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

MA = os.path.join(ROOT, "mapping-iterative-assembler_amd", "ma_hip")
HEADER = "/* map_alignment [V1.0] */ golden\n"
REGION = os.path.join(GOLDEN, "ma_region")


def malns():
    return sorted(os.path.basename(p) for p in os.listdir(os.path.join(GOLDEN, "maln")) if re.search(r"\.[0-9]$", p))


def recorded_runs():
    """{maln name: {run key: arguments}} of tests/golden/ma_region/runs.json: the runs every file gets, and "f6.<tag>" and
    "f61.<tag>" for each of its regions"""
    with open(os.path.join(REGION, "runs.json")) as f:
        rec = json.load(f)
    runs = {}
    for name, regions in rec["regions"].items():
        runs[name] = dict(rec["common"])
        for tag, arg in regions.items():
            for fmt in ("6", "61"):
                runs[name][f"f{fmt}.{tag}"] = ["-f", fmt] + (["-R", arg] if arg is not None else [])
    return runs


def test_every_maln_has_recorded_runs():
    runs = recorded_runs()
    assert sorted(runs) == malns()
    for name, r in runs.items():
        assert {"default", "f1c1", "f1c2", "f2c1", "f2c2", "f6.C", "f61.I"} <= set(r), name
        assert sum(1 for k in r if k.startswith("f6.R")) >= 7 and sum(1 for k in r if k.startswith("f61.R")) >= 7, name


@pytest.mark.parametrize("name", malns())
def test_ma_region_reports_identical(name, tmp_path):
    runs = recorded_runs()[name]
    with open(os.path.join(REGION, "hashes.json")) as f:
        hashes = json.load(f)
    with gzip.open(os.path.join(REGION, "outputs.json.gz")) as f:
        small = json.load(f)[name]
    full = str(tmp_path / name)
    with open(full, "w") as f:
        f.write(HEADER + open(os.path.join(GOLDEN, "maln", name)).read())

    def run(key):
        return key, subprocess.run([MA, "-M", full] + runs[key], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)

    with ThreadPoolExecutor(max_workers=6) as pool:      # (six processes with the GPU open at a time)
        results = list(pool.map(run, sorted(runs)))
    checked = 0
    for key, r in results:
        assert r.returncode == 0, (key, r.stderr[-300:])
        if key in small:
            assert r.stdout == small[key].encode("latin1"), key
        else:
            h = hashes.get(f"{name}.{key}")
            assert h is not None, f"no golden for {name}.{key}"
            assert (len(r.stdout), hashlib.sha256(r.stdout).hexdigest()) == (h["bytes"], h["sha256"]), key
        checked += 1
    assert checked == len(runs) and checked >= 21


# ---- the library call on a million records ------------------------------------------------------------------------------
N_REC, REF_LEN, SEED = 1_000_000, 16_619, 20261016
NARROW = (8_000, 8_299)


def synthetic_records():
    """About a million records on a 16 619-column reference: lengths 30..256, starts spread over the reference, three percent
    of them with one insert of 1..3 bases in front of one of their columns -- at one of 400 columns of the reference (inserts
    against a reference sit where the sample differs from it), some in front of their first column, where they do not count."""
    rng = np.random.default_rng(SEED)
    length = rng.integers(30, 257, size=N_REC).astype(np.int64)
    start = (rng.random(N_REC) * (REF_LEN - length + 1)).astype(np.int64)
    order = np.lexsort((start + length - 1, start))
    start, length = start[order], length[order]
    col_off = np.concatenate(([0], np.cumsum(length))).astype(np.int64)
    seq = np.frombuffer(b"ACGT-", dtype=np.uint8)[rng.choice(5, size=int(col_off[-1]), p=[0.24, 0.24, 0.24, 0.24, 0.04])]
    hot = np.sort(rng.choice(np.arange(1, REF_LEN), size=400, replace=False))
    # a record takes the first hot column it covers (its own first column included), if it is one of the three percent
    k = np.searchsorted(hot, start)
    k_ok = k < len(hot)
    col = hot[np.minimum(k, len(hot) - 1)]
    has = k_ok & (col < start + length) & (rng.random(N_REC) < 0.033)         # (nearly every record covers a hot column)
    ins_record = np.flatnonzero(has).astype(np.int32)
    ins_pos = (col[has] - start[has]).astype(np.int32)
    ins_len = rng.integers(1, 4, size=len(ins_record)).astype(np.int64)
    ins_off = np.concatenate(([0], np.cumsum(ins_len))).astype(np.int64)
    ins_bases = np.frombuffer(b"acgt", dtype=np.uint8)[rng.integers(0, 4, size=int(ins_off[-1]))]
    gaps = np.zeros(REF_LEN, dtype=np.int32)
    counts = ins_pos > 0                               # ref->gaps: the longest insert in front of a column, own first columns aside
    np.maximum.at(gaps, col[has][counts], ins_len[counts].astype(np.int32))
    return dict(start=start.astype(np.int32), length=length, col_off=col_off, seq=np.ascontiguousarray(seq), gaps=gaps, ins_record=ins_record,
                ins_pos=ins_pos, ins_off=ins_off, ins_bases=np.ascontiguousarray(ins_bases))


def expected_rows(d, first, last):
    end = d["start"].astype(np.int64) + d["length"] - 1
    return np.flatnonzero((d["start"] <= last) & (end >= first)).astype(np.int64)


def expected_row(d, r, first, last, colmap):
    """the row rule, one record: dots where the record is not; on its first column dots for the insert columns; on a later
    column its inserted bases, then '-' up to gaps; then its own character"""
    row = np.full(int(colmap[-1]), ord("."), dtype=np.uint8)
    s, n = int(d["start"][r]), int(d["length"][r])
    a, b = max(s, first), min(s + n - 1, last)
    if a > b:
        return row
    p = np.arange(a, b + 1)
    g = d["gaps"][p]
    at = colmap[p - first]
    row[at + g] = d["seq"][d["col_off"][r] + (p - s)]
    ins = {}
    for e in d["by_record"].get(int(r), ()):
        ins[int(d["ins_pos"][e])] = d["ins_bases"][d["ins_off"][e]:d["ins_off"][e + 1]]
    for i in np.flatnonzero(g > 0):
        if p[i] == s:
            continue
        bases = ins.get(int(p[i] - s), np.empty(0, np.uint8))
        row[at[i]:at[i] + g[i]] = ord("-")
        row[at[i]:at[i] + len(bases)] = bases
    return row


def test_region_of_a_million_records_matches_the_row_rule():
    import mia_amd
    d = synthetic_records()
    d["by_record"] = {}
    for e, r in enumerate(d["ins_record"]):
        d["by_record"].setdefault(int(r), []).append(e)
    ins_col = d["start"][d["ins_record"]].astype(np.int64) + d["ins_pos"]
    assert 0.02 * N_REC <= len(d["ins_record"]) <= 0.05 * N_REC and (d["ins_pos"] == 0).any() and int(d["gaps"].max()) == 3
    hip = mia_amd.MiaHip(0)
    hip.set_pssm(mia_amd.flat_pssm())
    smp = np.full(int(d["col_off"][-1]), ord("P"), dtype=np.uint8)
    hip.ma_tally(REF_LEN, d["gaps"], d["start"], np.zeros(N_REC, np.uint8), d["col_off"], d["seq"], smp, d["ins_record"], d["ins_pos"],
                 d["ins_off"], d["ins_bases"])
    del smp
    rng = np.random.default_rng(SEED + 1)
    for first, last in (NARROW, (0, REF_LEN - 1), (9_000, 8_900)):
        want = expected_rows(d, first, last)
        colmap = np.concatenate(([0], np.cumsum(d["gaps"][first:last + 1].astype(np.int64) + 1))) if first <= last else np.zeros(1, np.int64)
        hip.stage_stats(reset=True)
        rows, text = hip.ma_region(first, last)
        st = hip.stage_stats()
        assert st["k_ma_region_select"][1] == 1 and st["k_ma_region_render"][1] == (1 if len(want) and first <= last else 0)
        print("region %d..%d: %d rows x %d; k_ma_region_select %.3f ms, k_ma_region_render %.3f ms" %
              (first, last, len(want), int(colmap[-1]), st["k_ma_region_select"][0], st["k_ma_region_render"][0]))
        assert text.shape == (len(want), int(colmap[-1])), (first, last, text.shape)
        assert np.array_equal(rows, want), (first, last)
        if first > last:
            assert len(want) > 0 and text.shape[1] == 0
            continue
        # every row whose record has an insert inside the region, and random ones up to 5 000 at least
        bearing = np.flatnonzero(np.isin(want, d["ins_record"][(ins_col >= first) & (ins_col <= last) & (d["ins_pos"] > 0)]))
        assert len(bearing) >= 100, (first, last, len(bearing))
        sample = np.union1d(bearing, rng.choice(len(want), size=min(len(want), 5_000), replace=False))
        assert len(sample) >= min(len(want), 5_000)
        for i in sample:
            exp = expected_row(d, want[i], first, last, colmap)
            assert np.array_equal(text[i], exp), (first, last, int(i), int(want[i]))
        del text


# ---- the ordered selection at the edges of a workgroup's 1 024 records -------------------------------------------------------------
EDGE_REGION = (80, 190)                    # about half of make_records' records reach into it, and the insert columns of column 150 lie in it


@pytest.mark.parametrize("name", mc.SCAN_EDGES)
def test_region_around_one_workgroup_of_records_matches_the_row_rule(name):
    import mia_amd
    m = mc.make_case(name)
    d = ms.flatten(m)
    n = len(m.rec)
    d["length"] = np.diff(d["col_off"])
    d["by_record"] = {}
    for e, r in enumerate(d["ins_record"]):
        d["by_record"].setdefault(int(r), []).append(e)
    first, last = EDGE_REGION
    want = expected_rows(d, first, last)
    assert 0.35 * n <= len(want) <= 0.65 * n and want[-1] >= n - 8                      # the ranks of the compaction matter, up to the last records
    ins_col = d["start"][d["ins_record"]].astype(np.int64) + d["ins_pos"]
    assert len(np.intersect1d(want, d["ins_record"][(ins_col >= first) & (ins_col <= last)])) >= 20
    colmap = np.concatenate(([0], np.cumsum(d["gaps"][first:last + 1].astype(np.int64) + 1)))
    hip = mia_amd.MiaHip(0)
    hip.set_pssm(m.fpsm, m.rpsm)
    hip.ma_tally(*ms.ma_tally_args(d))
    rows, text = hip.ma_region(first, last)
    assert text.shape == (len(want), int(colmap[-1])) and np.array_equal(rows, want)
    for i in range(len(want)):
        assert np.array_equal(text[i], expected_row(d, want[i], first, last, colmap)), (name, i, int(want[i]))
