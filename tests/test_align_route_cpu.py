"""The route of an alignment without a GPU: csrc/align_route.h (plain C++17) is compiled into tests/align_route_driver.cpp and asked
about every combination of its inputs.  `restate` below is the PARENT's align_all, expression by expression (the many-rejects rule
three times over, as it stood there), in numpy; every field of AlignRoute must agree with it for every input.  The named cases pin the
routes of the benched workloads: their fields are written out here from DESIGN 3.1 / 3.5 and profiles/r06/*_timeline.txt."""
import itertools
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

# (name, bits) in the driver's order
FIELDS = [("nwords", 3), ("bx", 1), ("run_filter", 1), ("fused_prep", 1), ("filtered", 1), ("kocc", 1), ("banded", 1), ("want_bits", 1), ("new_flow", 1),
          ("split", 1), ("fork_by_launch", 1), ("fine", 1), ("many_rejects", 1), ("planner_head_first", 1), ("direct_open", 1), ("maxw", 7), ("quick", 1),
          ("quick_lds", 1), ("one_launch", 1), ("fork_at_quick", 1), ("qch", 4), ("quick_phase", 3), ("full_first", 3), ("full_last", 3), ("grid_cap", 9),
          ("three_streams", 1), ("two_streams", 1), ("values_aside", 1), ("trace_signals", 1), ("planner_aside", 1), ("use_plain", 1), ("plan_count_late", 1)]
DEFAULTS = dict(n=1, max_len=100, wrap=16875, L=16619, plane_words=281, kh_entries=0, flat=1, ref_mostly_bases=1, ref_few_n=1, bx_ok=1, explicit_win=0,
                deferred=0, pend_encode=0, own_umax=1, rejects=0, use_filter=1, use_banddp=1, use_bx=1, use_lanes=1, use_fine=1, use_quick=1, bx_serial=0,
                plan_split=1, use_direct_open=1, no_prep_fuse=0, ext_events=31, dbg=0, bx_dbg=0)
BX_QCH, BX_MAXW = 8, 64


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("align_route") / "align_route_driver"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-o", str(exe), os.path.join(ROOT, "tests", "align_route_driver.cpp")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()
    return str(exe)


def ask(driver, axes, cfgs):
    """axes: [(field, values)], cfgs: [dict of fields]: the driver's two words per point, cfg-major, first axis slowest"""
    names = sorted(DEFAULTS)
    text = "axes %d\n" % len(axes) + "".join("%s %s\n" % (k, " ".join(str(int(v)) for v in vs)) for k, vs in axes)
    text += "cfgs %d %s\n" % (len(cfgs), " ".join(names)) + "".join(" ".join(str(int({**DEFAULTS, **c}[k])) for k in names) + "\n" for c in cfgs)
    out = subprocess.run([driver], input=text.encode(), check=True, stdout=subprocess.PIPE, timeout=300).stdout
    w = np.frombuffer(out, np.uint64).reshape(-1, 2)
    assert len(w) == len(cfgs) * int(np.prod([len(vs) for _, vs in axes]))
    return w


def unpack(word):
    out, at = {}, 0
    for name, bits in FIELDS:
        out[name] = (word >> np.uint64(at)) & np.uint64((1 << bits) - 1)
        at += bits
    return out


def restate(i):
    """the parent's align_all over arrays of inputs (dict of int64 arrays); what a branch it does not reach would have set is 0"""
    B = lambda x: np.asarray(x).astype(bool)
    n, words = i["n"], i["plane_words"]
    flat, rmb, deferred = B(i["flat"]), B(i["ref_mostly_bases"]), B(i["deferred"])
    dbg, bxd, ext = i["dbg"], i["bx_dbg"], i["ext_events"]
    filter_ok = flat & B(i["use_filter"]) & rmb
    bx = B(i["bx_ok"]) & B(i["use_bx"]) & (rmb | (i["kh_entries"] > 0)) & (i["wrap"] <= (1 << 22)) & ~B(dbg & 128)
    run_filter = filter_ok & ~bx
    fused_prep = B(i["pend_encode"]) & bx & ~B(i["no_prep_fuse"])
    filtered = run_filter | bx
    kocc = filtered & (i["wrap"] <= (1 << 22)) & ~bx
    banded = filtered & (bx | (B(i["use_banddp"]) & kocc & ~B(dbg & 128)))
    want_bits = bx & B(i["use_quick"]) & ((i["kh_entries"] <= 0) | B(i["ref_few_n"]))
    new_flow = bx & B(i["use_lanes"]) & ~B(i["bx_serial"]) & ~B(dbg & 256) & ~B(i["explicit_win"])
    split = bx & B(i["plan_split"])
    fork_by_launch = B(ext & 1) & new_flow & ~B(dbg & 256)
    rejects_before = i["rejects"]
    fine = split & B(i["use_fine"]) & ((i["use_fine"] > 1) | ~flat | (n >= 4000000) | ~rmb | (rejects_before * 20 > n))
    last_phase = np.where(split, np.where(fine, 3, 2), 0)
    lr = i["rejects"]
    many_early = ~rmb | (lr * 20 > n)
    planner_head_first = new_flow & deferred & many_early & ~B(dbg & 256)
    direct_open = new_flow & deferred & B(i["use_direct_open"]) & ~many_early & ~planner_head_first & ~B(dbg & 256) & ~B(bxd & 12)
    maxw = np.where(B(i["use_lanes"]), BX_MAXW, 32)
    maxw = np.where(~fine & (i["use_fine"] < 2), 32, maxw)
    quick = split & new_flow & want_bits & ~B(bxd & 32) & B(i["own_umax"]) & (~fine | (n >= 2000000) | (i["use_quick"] > 1))
    fork_at_quick = quick & deferred & direct_open & ~fine & ~planner_head_first & ~B(bxd & 12)
    quick_lds = quick & (words * 24 <= 38 * 1024)
    one_launch = quick & ~fine
    qch = np.where(quick & (n >= 4000000) & (words * 24 <= 16 * 1024), BX_QCH, 4)
    phase_first = np.where(split & ~one_launch, 1, 0)
    phase_last = np.where(one_launch, 0, last_phase)
    kern = lambda ph: np.where(one_launch & (ph == 0), 6, ph)      # (phase 0 of the looped launch is the instance <NW, 6>)
    g = (n + 255) // 256
    grid = lambda ph: np.where(ph >= 2, np.minimum(g, 1024), np.where(one_launch, np.minimum(g, 256), g))
    three = new_flow & ~B(dbg & 256)
    two = bx & ~new_flow & ~B(dbg & 256)
    last_rejects = i["rejects"]
    many_rejects = bx & (~rmb | (last_rejects * 20 > n))
    r = dict(nwords=(i["max_len"] + 63) >> 6, bx=bx, run_filter=run_filter, fused_prep=fused_prep, filtered=filtered, kocc=kocc, banded=banded,
             want_bits=want_bits, new_flow=new_flow, split=split, fork_by_launch=fork_by_launch, fine=fine, many_rejects=many_rejects,
             planner_head_first=planner_head_first, direct_open=direct_open, maxw=np.where(bx, maxw, 0), quick=quick, quick_lds=quick_lds,
             one_launch=one_launch, fork_at_quick=fork_at_quick, qch=qch, quick_phase=np.where(quick, np.where(quick_lds, 5, 4), 0),
             full_first=np.where(bx, kern(phase_first), 0), full_last=np.where(bx, kern(phase_last), 0), grid_cap=np.where(one_launch, 256, 0),
             three_streams=three, two_streams=two, values_aside=three & ~(deferred & ~fork_at_quick), trace_signals=three & B(ext & 2) & ~B(bxd & 8),
             planner_aside=three & deferred, use_plain=~banded | many_rejects, plan_count_late=~planner_head_first & ~direct_open)
    grids = (np.where(bx, grid(phase_first), g), np.where(bx, grid(phase_last), g))
    # ONE PREDICATE: what `fine`, `planner_head_first` / `direct_open` and `use_plain` were each told about the rejects
    assert np.array_equal(many_early, ~rmb | (rejects_before * 20 > n)) and np.array_equal(many_rejects, bx & many_early)
    return r, grids


def switch_settings():
    """what read_alt_switches makes of every variable a test or tool sets (one at a time, and two at a time)"""
    one = [dict(use_filter=0, use_bx=0), dict(use_banddp=0, use_bx=0), dict(use_bx=0), dict(use_lanes=0), dict(bx_serial=1), dict(plan_split=0),
           dict(use_fine=0), dict(use_fine=2), dict(use_quick=0), dict(use_quick=2), dict(use_direct_open=0), dict(no_prep_fuse=1), dict(ext_events=0),
           dict(dbg=128), dict(dbg=256), dict(dbg=4096), dict(bx_dbg=4), dict(bx_dbg=8), dict(bx_dbg=5), dict(bx_dbg=32), dict(bx_dbg=64), dict(bx_dbg=128),
           dict(bx_dbg=512)]
    cfgs = [dict()] + one
    for a, b in itertools.combinations(one, 2):
        if not set(a) & set(b):
            cfgs.append({**a, **b})
    return cfgs


BOOLS = ["flat", "ref_mostly_bases", "ref_few_n", "bx_ok", "explicit_win", "deferred", "pend_encode", "own_umax"]
NS = [1, 1999999, 2000000, 3999999, 4000000]


def test_every_route_agrees_with_the_parents_expressions(driver):
    # plane words on both sides of 16 KB (682 | 683 words of 24 bytes) and of 38 KB (1 621 | 1 622); wrap on both sides of 1 << 22
    axes = [(b, [0, 1]) for b in BOOLS] + [("kh_entries", [0, 40]), ("plane_words", [682, 683, 1621, 1622]), ("wrap", [1 << 22, (1 << 22) + 1])]
    cfgs = switch_settings()
    checked = 0
    for n in NS:
        for step in (0, 1):
            rej = n // 20 + step
            w_axes = [("n", [n]), ("rejects", [rej])] + axes
            w = ask(driver, w_axes, cfgs)
            mesh = np.meshgrid(*[np.asarray(vs, np.int64) for _, vs in w_axes], indexing="ij")
            per = mesh[0].size
            for c, cfg in enumerate(cfgs):
                inp = {k: np.full(per, v, np.int64) for k, v in {**DEFAULTS, **cfg}.items()}
                for (k, _), m in zip(w_axes, mesh):
                    inp[k] = m.reshape(-1)
                got = unpack(w[c * per:(c + 1) * per, 0])
                want, grids = restate(inp)
                for name, _ in FIELDS:
                    bad = np.flatnonzero(got[name].astype(np.int64) != np.asarray(want[name]).astype(np.int64))
                    assert bad.size == 0, (name, cfg, {k: int(v[bad[0]]) for k, v in inp.items()}, int(got[name][bad[0]]))
                g = w[c * per:(c + 1) * per, 1]
                assert np.array_equal((g & np.uint64(0xFFFFFFFF)).astype(np.int64), grids[0]), cfg
                assert np.array_equal((g >> np.uint64(32)).astype(np.int64), grids[1]), cfg
                checked += per
    assert checked == len(NS) * 2 * 256 * 2 * 4 * 2 * len(cfgs) and len(cfgs) > 200


def test_read_lengths(driver):
    lens = [64, 65, 128, 129, 192, 193, 256]
    w = ask(driver, [("deferred", [0, 1]), ("flat", [0, 1]), ("n", NS), ("max_len", lens)], [dict()])
    got = unpack(w[:, 0])["nwords"].reshape(2, 2, len(NS), len(lens))
    assert (got == np.array([1, 2, 2, 3, 3, 4, 4], np.uint64)).all()


def route(driver, **inputs):
    w = ask(driver, [], [inputs])
    r = {k: int(v[0]) for k, v in unpack(w[:, 0]).items()}
    r["grids"] = (int(w[0, 1]) & 0xFFFFFFFF, int(w[0, 1]) >> 32)
    return r


def has(r, **fields):
    assert {k: r[k] for k in fields} == fields


# mt311 wrapped: 16 619 + 256 columns, 281 words per plane (6.7 KB for the three).  mia_hip_iterate: deferred, the reference comes as ASCII.
STEP = dict(deferred=1, pend_encode=1, wrap=16875, L=16619, plane_words=281)


def test_configs1_steady(driver):
    r = route(driver, n=1000000, flat=1, rejects=3000, **STEP)
    has(r, bx=1, fused_prep=1, quick=1, quick_phase=5, quick_lds=1, qch=4, fine=0, one_launch=1, full_first=6, full_last=6, grid_cap=256,
        direct_open=1, fork_at_quick=1, maxw=32, use_plain=0, many_rejects=0, planner_head_first=0, plan_count_late=0, three_streams=1,
        values_aside=1, planner_aside=1, fork_by_launch=1, trace_signals=1, nwords=2, run_filter=0)
    assert r["grids"] == (256, 256)


def test_configs1_first_iteration(driver):
    # mt311 itself: N in every other column, the table spells none of them out
    r = route(driver, n=1000000, flat=1, rejects=0, ref_mostly_bases=0, ref_few_n=0, kh_entries=30000, **STEP)
    has(r, bx=1, quick=0, quick_phase=0, fine=1, full_first=1, full_last=3, planner_head_first=1, use_plain=1, many_rejects=1, direct_open=0,
        fork_at_quick=0, maxw=64, plan_count_late=0, values_aside=0, planner_aside=1, want_bits=0)
    assert r["grids"] == (3907, 1024)


def test_configs2_steady(driver):
    r = route(driver, n=1000000, flat=0, rejects=20000, **STEP)
    has(r, bx=1, fine=1, quick=0, full_first=1, full_last=3, direct_open=1, fork_at_quick=0, values_aside=0, use_plain=0, maxw=64, plan_count_late=0)


def test_configs3_steady_and_its_eighth(driver):
    r = route(driver, n=10000000, flat=0, rejects=200000, max_len=100, **STEP)
    has(r, quick=1, quick_phase=5, qch=BX_QCH, fine=1, one_launch=0, full_first=1, full_last=3, fork_at_quick=0, direct_open=1, values_aside=0)
    assert r["grids"] == (39063, 1024)
    has(route(driver, n=1250000, flat=0, rejects=25000, **STEP), quick=0, quick_phase=0, fine=1, full_first=1, full_last=3)


def test_configs4(driver):
    # 5 M reads of 150 bases, a linear reference of 100 kb with two N columns: 1 580 words per plane, 37.9 KB for the three
    r = route(driver, n=5000000, flat=0, max_len=150, rejects=100000, deferred=1, pend_encode=1, wrap=100000, L=100000, plane_words=1580,
              kh_entries=80, ref_few_n=1)
    assert 1580 * 24 <= 38 * 1024 < 1622 * 24
    has(r, want_bits=1, quick=1, quick_phase=5, quick_lds=1, qch=4, nwords=3, fine=1, fork_at_quick=0)
    has(route(driver, n=5000000, flat=0, max_len=150, deferred=1, wrap=100000, L=100000, plane_words=1580, kh_entries=80, ref_few_n=0), want_bits=0, quick=0)


def test_realign_and_align_windows(driver):
    r = route(driver, n=1000000, flat=1, rejects=3000, deferred=0, wrap=16875, L=16619, plane_words=281)
    has(r, bx=1, fused_prep=0, quick=1, direct_open=0, fork_at_quick=0, three_streams=1, values_aside=1, planner_aside=0, plan_count_late=1, full_first=6)
    w = route(driver, n=1000000, flat=1, deferred=0, explicit_win=1, own_umax=0, wrap=3000000, L=3000000, plane_words=46892)
    has(w, bx=1, new_flow=0, three_streams=0, two_streams=1, quick=0, direct_open=0, planner_aside=0, full_first=1, full_last=2)


def test_round1_and_full_window_routes(driver):
    r = route(driver, n=1000000, flat=1, use_bx=0, **STEP)                      # MIA_HIP_NO_BANDX, flat matrix
    has(r, bx=0, run_filter=1, kocc=1, banded=1, fused_prep=0, use_plain=0, three_streams=0, two_streams=0, quick=0, plan_count_late=1, filtered=1)
    r = route(driver, n=1000000, flat=1, use_filter=0, use_bx=0, **STEP)        # MIA_HIP_NO_DIAG_FILTER
    has(r, bx=0, run_filter=0, filtered=0, kocc=0, banded=0, use_plain=1, three_streams=0, two_streams=0, quick=0, plan_count_late=1, fused_prep=0)
