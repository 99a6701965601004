"""The route of pass 1 without a GPU: csrc/pass1_route.h (plain C++17) is compiled into tests/pass1_route_driver.cpp and asked about a grid
of inputs.  `restate` below is the PARENT's mia_hip_pass1, expression by expression (`len1 <= (1 << 22)` three times and
`p1_other * 50 <= L` twice, as they stood there), in numpy; every field of Pass1Route must agree with it on every point.  The named cases
pin the routes of what is benched (bench.py's five pass-1 labels) and tested (test_gpu_pass1.py), their fields written out by hand
from the code and DESIGN 3.5.  The driver also prints the reverse-complement function that replaced a table literal, for all 256 bytes."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

IN_FIELDS = ["n", "max_len", "L", "circular", "kmer_len", "max_pos", "flat", "bx_ok", "use_bx", "use_filter", "p1_other", "wild_entries", "waves_cu", "cus",
             "has_cpl", "alt_cpl", "has_plain", "alt_plain"]
OUT_FIELDS = ["wl", "wrap", "len1", "cpl", "plain", "ch", "nch", "mask_words", "lds", "rows_p", "trace_bytes", "ckpt_words", "waves_cu", "grid", "fast_ok",
              "gen_ok", "filtered", "want_wild", "anchored_ok", "need_todo", "need_ktab", "rebuild_ktab_for_anchors", "ref_mostly_bases", "wild",
              "wild_entries", "refusal", "code", "wants_wild_helper"]
DEFAULTS = dict(n=200000, max_len=100, L=16619, circular=1, kmer_len=-1, max_pos=200, flat=1, bx_ok=1, use_bx=1, use_filter=1, p1_other=0, wild_entries=0,
                waves_cu=12, cus=256, has_cpl=0, alt_cpl=0, has_plain=0, alt_plain=0)
# the constants' owners: mia_layout.h, pass1_body.h, bandx_body.h, include/mia_hip.h
GOP, GEP, MAX_READ, WAVE, P1_IDXM, NARROW, WIDE, BX_WILD, ERR_RANGE = 1000, 200, 256, 64, 1023, 4, 12, 3, -3
NONE, HORIZON, KMER_TABLE, LDS = 0, 1, 2, 3
MESSAGES = ["PSSM too large for the pass-1 candidate horizon", "reference too long for the k-mer table", "reference too long for the pass-1 LDS masks"]
MAX_POS_FLAT, MAX_POS_ANCIENT, MAX_POS_SOLEXA = 200, 251, 250      # largest positive entry of the flat matrix and of the two shipped ones


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("pass1_route") / "pass1_route_driver"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-o", str(exe), os.path.join(ROOT, "tests", "pass1_route_driver.cpp")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()
    return str(exe)


def ask(driver, inp):
    """inp: dict of equally long int64 arrays; the route's fields as a dict of int64 arrays"""
    rec = np.stack([np.asarray(inp[k], np.int64) for k in IN_FIELDS], axis=1)
    out = subprocess.run([driver, "route"], input=np.ascontiguousarray(rec).tobytes(), check=True, stdout=subprocess.PIPE, timeout=300).stdout
    w = np.frombuffer(out, np.int64).reshape(-1, len(OUT_FIELDS))
    assert len(w) == len(rec)
    return {k: w[:, j] for j, k in enumerate(OUT_FIELDS)}


def rel(cpl):
    return P1_IDXM + 1 - WAVE * cpl


def restate(i):
    """the parent's mia_hip_pass1 over arrays of inputs, in its order; what a branch it does not reach would have set is 0"""
    B = lambda x: np.asarray(x).astype(bool)
    n, L, kmer_len, max_len, max_pos = i["n"], i["L"], i["kmer_len"], i["max_len"], i["max_pos"]
    circular, flat = B(i["circular"]), B(i["flat"])
    wl = np.where(circular, np.where(L < MAX_READ, L, MAX_READ), 0)
    wrap = L + wl
    len1 = np.where(circular, wrap, L)
    horizon_ok = lambda r: max_len * max_pos + (GOP + GEP * (max_len + 1)) < (GOP + GEP * (r - 1))
    cpl = np.where((kmer_len <= 0) & horizon_ok(rel(WIDE)), WIDE, NARROW)
    want = i["alt_cpl"]
    cpl = np.where(B(i["has_cpl"]) & (((want == WIDE) & horizon_ok(rel(WIDE))) | (want == NARROW)), want, cpl)
    refuse_horizon = ~horizon_ok(rel(cpl))
    P1_CH = WAVE * cpl
    plain = np.where(B(i["has_plain"]), (i["alt_plain"] != 0).astype(np.int64), 1)
    refuse_ktab = (kmer_len > 0) & (wrap >= (1 << 24))
    nch = (len1 + P1_CH - 1) // P1_CH
    mask_words = np.where(kmer_len > 0, nch * (P1_CH // 32) + 4, 0)
    lds = MAX_READ * 10 + 5 * MAX_READ * 4 + 2 * mask_words * 4
    rows_p = (max_len + 3) & ~3
    trace_bytes, ckpt_words = rows_p * P1_CH * 2, 2 * nch * 5 * rows_p
    refuse_lds = lds > 160 * 1024
    waves_cu = np.where(i["waves_cu"] > 4, i["waves_cu"] & ~3, i["waves_cu"])
    grid = np.minimum(i["cus"] * waves_cu, n)
    p1_other = i["p1_other"]
    fast_ok = flat & B(i["use_filter"]) & (kmer_len <= 0) & (len1 >= max_len)
    gen_ok = ~flat & B(i["bx_ok"]) & B(i["use_bx"]) & B(i["use_filter"]) & (kmer_len <= 0) & (len1 >= max_len)
    filtered = fast_ok & (p1_other * 50 <= L)
    walked = (fast_ok | gen_ok) & B(p1_other) & (len1 <= (1 << 22))
    wild_entries = np.where(walked, i["wild_entries"], 0)
    wild_entries = np.where(wild_entries > (1 << 24), 0, wild_entries)
    anchored_ok = (fast_ok | gen_ok) & ((p1_other == 0) | (wild_entries > 0)) & (len1 <= (1 << 22))
    need_todo = filtered | anchored_ok
    need_ktab = need_todo & (len1 <= (1 << 22))
    anchors_run = anchored_ok & need_ktab                  # (... && n_dp > 0: the reads' business)
    rebuild = anchors_run & (B(p1_other) | ~filtered)
    wild = np.where(rebuild & B(p1_other), BX_WILD, 0)
    lent_ref_mostly_bases = p1_other * 50 <= L
    refusal = np.where(refuse_horizon, HORIZON, np.where(refuse_ktab, KMER_TABLE, np.where(refuse_lds, LDS, NONE)))
    return dict(wl=wl, wrap=wrap, len1=len1, cpl=cpl, plain=plain, ch=P1_CH, nch=nch, mask_words=mask_words, lds=lds, rows_p=rows_p,
                trace_bytes=trace_bytes, ckpt_words=ckpt_words, waves_cu=waves_cu, grid=grid, fast_ok=fast_ok, gen_ok=gen_ok, filtered=filtered,
                want_wild=walked, anchored_ok=anchored_ok, need_todo=need_todo, need_ktab=need_ktab, rebuild_ktab_for_anchors=rebuild,
                ref_mostly_bases=lent_ref_mostly_bases, wild=wild, wild_entries=wild_entries, refusal=refusal,
                code=np.where(refusal == NONE, 0, ERR_RANGE), wants_wild_helper=walked)


def flip(max_len, cpl):
    """the largest max_pos for which horizon_ok(rel(cpl)) still holds with reads of max_len (never below 0)"""
    return np.maximum((GEP * (rel(cpl) - 2 - max_len) - 1) // max_len, 0)


def resolve(pts):
    """the axes that are given relative to another input: max_pos (>= 1000: flip point of NARROW / WIDE plus 0 | 1), p1_other (index)"""
    i = {k: np.asarray(v, np.int64).copy() for k, v in pts.items()}
    sel = i["max_pos"]
    for code, cpl in ((1000, NARROW), (2000, WIDE)):
        for step in (0, 1):
            i["max_pos"] = np.where(sel == code + step, flip(i["max_len"], cpl) + step, i["max_pos"])
    sel, L = i["p1_other"].copy(), i["L"]
    i["p1_other"] = np.where(sel == 2, L // 50, np.where(sel == 3, L // 50 + 1, sel))
    return i


AXES = dict(kmer_len=[-1, 0, 8, 12, 14], max_len=[1, 23, 24, 100, 256],
            max_pos=[MAX_POS_FLAT, MAX_POS_ANCIENT, MAX_POS_SOLEXA, 1000, 1001, 2000, 2001],
            L=[50, 600, 16619, 100000, (1 << 22) - 300, 1 << 22, (1 << 22) + 1, 1 << 24], circular=[0, 1], flat=[0, 1], bx_ok=[0, 1], use_bx=[0, 1],
            use_filter=[0, 1], p1_other=[0, 1, 2, 3], wild_entries=[0, 1, 1 << 24, (1 << 24) + 1],
            cpl_switch=[(0, 0), (1, 4), (1, 12), (1, 7)], plain_switch=[(0, 0), (1, 0), (1, 1)], waves_cu=[1, 4, 5, 13])


def points(names, rng=None, count=0):
    """the product of the named axes (the others at their defaults), or `count` points drawn from all axes at once"""
    if rng is None:
        mesh = np.meshgrid(*[np.arange(len(AXES[k])) for k in names], indexing="ij")
        idx = {k: m.reshape(-1) for k, m in zip(names, mesh)}
        size = mesh[0].size
    else:
        idx = {k: rng.integers(0, len(AXES[k]), count) for k in AXES}
        size = count
    pts = {k: np.full(size, v, np.int64) for k, v in DEFAULTS.items()}
    for k, at in idx.items():
        vals = np.asarray(AXES[k], np.int64)[at]
        if k == "cpl_switch":
            pts["has_cpl"], pts["alt_cpl"] = vals[:, 0], vals[:, 1]
        elif k == "plain_switch":
            pts["has_plain"], pts["alt_plain"] = vals[:, 0], vals[:, 1]
        else:
            pts[k] = vals
    return resolve(pts)


def compare(driver, inp):
    got, want = ask(driver, inp), restate(inp)
    for name in OUT_FIELDS:
        bad = np.flatnonzero(got[name] != np.asarray(want[name]).astype(np.int64))
        assert bad.size == 0, (name, {k: int(v[bad[0]]) for k, v in inp.items()}, int(got[name][bad[0]]), int(np.asarray(want[name])[bad[0]]))
    return got


def test_the_flip_points_are_flip_points():
    for cpl in (NARROW, WIDE):
        for max_len in AXES["max_len"]:
            ok = lambda mp: max_len * mp + (GOP + GEP * (max_len + 1)) < GOP + GEP * (rel(cpl) - 1)
            f = int(flip(np.int64(max_len), cpl))
            assert (ok(f) and not ok(f + 1)) or (f == 0 and not ok(0)), (cpl, max_len, f)


def test_every_route_agrees_with_the_parents_expressions(driver):
    # sizes, chunk width, grid and refusals: everything they read, crossed
    a = points(["kmer_len", "max_len", "max_pos", "L", "circular", "cpl_switch", "plain_switch", "waves_cu"])
    got = compare(driver, a)
    assert len(a["n"]) == 5 * 5 * 7 * 8 * 2 * 4 * 3 * 4
    assert set(got["refusal"]) == {NONE, HORIZON, KMER_TABLE, LDS} and set(got["cpl"]) == {NARROW, WIDE} and set(got["plain"]) == {0, 1}
    # the shortcuts in front of the DP: everything THEY read, crossed
    b = points(["kmer_len", "max_len", "L", "circular", "flat", "bx_ok", "use_bx", "use_filter", "p1_other", "wild_entries"])
    got = compare(driver, b)
    assert len(b["n"]) == 5 * 5 * 8 * 2 * 16 * 4 * 4
    for f in ("fast_ok", "gen_ok", "filtered", "want_wild", "anchored_ok", "need_todo", "need_ktab", "rebuild_ktab_for_anchors", "ref_mostly_bases"):
        assert set(got[f]) == {0, 1}, f
    assert set(got["wild"]) == {0, BX_WILD} and ((got["need_todo"] == 1) & (got["need_ktab"] == 0)).any()
    # ... and both groups at once: points drawn from the product of all the axes, with few reads too (the grid's other bound)
    c = points(None, np.random.default_rng(1), 400000)
    c["n"] = np.where(np.arange(400000) % 3 == 0, 150, c["n"])
    compare(driver, c)


def test_refusal_messages(driver):
    out = subprocess.run([driver, "messages"], check=True, stdout=subprocess.PIPE).stdout.decode().splitlines()
    assert out == MESSAGES


def route(driver, **inputs):
    got = ask(driver, resolve({k: np.array([v], np.int64) for k, v in {**DEFAULTS, **inputs}.items()}))
    return {k: int(v[0]) for k, v in got.items()}


def has(r, **fields):
    assert {k: r[k] for k in fields} == fields


# mt311: 16 619 columns, circular: 16 875 with the wrapped stretch.  As it is it carries an ambiguity code in every tenth column
# (1 705 of them, more than 2 %: the diagonal filter has nothing to decide, the anchors' tables spell the codes out); "plain_ref" has them resolved.
MT311 = dict(L=16619, circular=1, n=200000, max_len=100)
# LDS without masks: the substitution table and five carry arrays
LDS0 = 256 * 10 + 5 * 256 * 4


def test_bench_k12(driver):
    r = route(driver, kmer_len=12, max_pos=MAX_POS_FLAT, flat=1, p1_other=1705, **MT311)
    # masked sweep: narrow chunks (66 of them), masks of both strands in LDS; no shortcut in front of a masked DP
    has(r, refusal=NONE, wrap=16875, len1=16875, cpl=NARROW, ch=256, nch=66, mask_words=66 * 8 + 4, lds=LDS0 + 2 * (66 * 8 + 4) * 4, rows_p=100,
        trace_bytes=100 * 256 * 2, ckpt_words=2 * 66 * 5 * 100, fast_ok=0, gen_ok=0, filtered=0, anchored_ok=0, need_todo=0, need_ktab=0, want_wild=0,
        wild=0, plain=1, waves_cu=12, grid=256 * 12)


def test_bench_no_kmer_against_mt311(driver):
    r = route(driver, max_pos=MAX_POS_FLAT, flat=1, p1_other=1705, wild_entries=30000, **MT311)
    # wide chunks (22), no masks; the filter is skipped, the anchored windows run on tables that are rebuilt with the N columns spelled out
    has(r, refusal=NONE, cpl=WIDE, ch=768, nch=22, mask_words=0, lds=LDS0, fast_ok=1, gen_ok=0, ref_mostly_bases=0, filtered=0, want_wild=1,
        wild_entries=30000, anchored_ok=1, need_todo=1, need_ktab=1, rebuild_ktab_for_anchors=1, wild=BX_WILD, plain=1, trace_bytes=100 * 768 * 2)


def test_bench_no_kmer_plain_ref(driver):
    r = route(driver, max_pos=MAX_POS_FLAT, flat=1, p1_other=0, **MT311)
    # the filter first, the anchored windows behind it on the filter's own tables (no N column: nothing to rebuild)
    has(r, refusal=NONE, cpl=WIDE, fast_ok=1, filtered=1, ref_mostly_bases=1, want_wild=0, anchored_ok=1, need_todo=1, need_ktab=1,
        rebuild_ktab_for_anchors=0, wild=0)


def test_bench_ancient_no_kmer(driver):
    r = route(driver, max_pos=MAX_POS_ANCIENT, flat=0, bx_ok=1, p1_other=1705, wild_entries=30000, **MT311)
    # a position-specific matrix: no diagonal filter, the anchored windows in losses
    has(r, refusal=NONE, cpl=WIDE, fast_ok=0, gen_ok=1, filtered=0, want_wild=1, anchored_ok=1, need_todo=1, need_ktab=1, rebuild_ktab_for_anchors=1,
        wild=BX_WILD, ref_mostly_bases=0)


def test_bench_ancient_no_kmer_plain_ref(driver):
    r = route(driver, max_pos=MAX_POS_ANCIENT, flat=0, bx_ok=1, p1_other=0, **MT311)
    # no filter made the tables: they are built for the anchors, without spellings
    has(r, refusal=NONE, cpl=WIDE, gen_ok=1, filtered=0, want_wild=0, anchored_ok=1, need_todo=1, need_ktab=1, rebuild_ktab_for_anchors=1, wild=0,
        ref_mostly_bases=1)


def test_fixture_c_k8M_and_fixture_lin(driver):
    # test_gpu_pass1.py: tr1.fna (120 columns, no N), tf.fna's 25 reads (3 .. 256 bases), the flat matrix
    tf = dict(L=120, max_len=256, n=25, max_pos=MAX_POS_FLAT, flat=1)
    r = route(driver, circular=1, kmer_len=8, **tf)
    # the whole reference is wrapped once more (120 < 256); one narrow chunk with its masks
    has(r, refusal=NONE, wl=120, wrap=240, len1=240, cpl=NARROW, ch=256, nch=1, mask_words=12, lds=LDS0 + 96, rows_p=256, trace_bytes=256 * 256 * 2,
        ckpt_words=2 * 5 * 256, fast_ok=0, anchored_ok=0, need_todo=0, grid=25)
    r = route(driver, circular=0, kmer_len=-1, **tf)
    # reads of 256 bases leave the wide chunks' horizon of 256 columns no room: narrow chunks; a strand shorter than the longest read: no shortcut
    has(r, refusal=NONE, wl=0, wrap=120, len1=120, cpl=NARROW, nch=1, mask_words=0, lds=LDS0, fast_ok=0, filtered=0, anchored_ok=0, need_todo=0,
        need_ktab=0, rows_p=256, grid=25)


def test_reverse_complement_of_every_byte(driver):
    out = subprocess.run([driver, "revcom"], check=True, stdout=subprocess.PIPE).stdout
    assert len(out) == 256
    tbl = b"TVGH\0\0CD\0\0M\0KN\0\0\0YSAABWXR\0"      # the parent's literal, 'A' .. 'Z'
    assert len(tbl) == 26

    def old(b):
        r = 0
        if b == ord("-"):
            return b
        if ord("A") <= b <= ord("Z"):
            r = tbl[b - ord("A")]
        elif ord("a") <= b <= ord("z"):
            r = tbl[b - ord("a")] + 32
        return r if r else ord("N")

    assert out == bytes(old(b) for b in range(256))
