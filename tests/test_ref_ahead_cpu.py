"""Reference ahead without a GPU: csrc/ref_ahead.h (when may the tables prepared behind the last consensus stand in for this call's?)
and the ref_ready input of csrc/align_route.h, both plain C++17, compiled into tests/ref_ahead_driver.cpp.

The hit/miss function is enumerated: every key field differing alone, the string differing in its last byte, another length, another
circular flag.  The route with ref_ready is asked over the inputs tests/test_align_route_cpu.py enumerates: prep_none is set exactly
where ref_ready meets the band pipeline, and nothing else of the route moves."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_align_route_cpu import BOOLS, DEFAULTS, NS, switch_settings, unpack

KEY_FIELDS = ["L", "circular", "n_other", "kh_entries", "kslots", "kwild", "plane_words", "nib_words", "bits"]
# mt311's consensus, circular: 16 569 + 256 columns; a second key with N columns spelled out
KEYS = [dict(L=40, circular=1, n_other=0, kh_entries=0, kslots=65536, kwild=0, plane_words=281, nib_words=2130, bits=1),
        dict(L=40, circular=0, n_other=3, kh_entries=212, kslots=131072, kwild=3, plane_words=9, nib_words=40, bits=0)]
OTHER = dict(L=39, circular=None, n_other=1, kh_entries=64, kslots=262144, kwild=1, plane_words=282, nib_words=2131, bits=None)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("ref_ahead") / "ref_ahead_driver"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-o", str(exe), os.path.join(ROOT, "tests", "ref_ahead_driver.cpp")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()
    return str(exe)


def ask_hit(driver, cases):
    """cases: [(built, want, kept, new)] -> [(same_string, hit)]"""
    text = "".join("%s %s %s %s\n" % (" ".join(str(int(b[k])) for k in KEY_FIELDS), " ".join(str(int(w[k])) for k in KEY_FIELDS), kept, new)
                   for b, w, kept, new in cases)
    out = subprocess.run([driver, "hit"], input=text.encode(), check=True, stdout=subprocess.PIPE, timeout=60).stdout.decode().split("\n")
    got = [tuple(int(x) for x in line.split()) for line in out if line]
    assert len(got) == len(cases)
    return got


def test_hit_needs_the_same_key_and_the_same_string(driver):
    rng = np.random.default_rng(5)
    for key in KEYS:
        s = "".join(rng.choice(list("ACGTN"), key["L"]))
        cases, want_hit = [(key, dict(key), s, s)], [(1, 1)]
        # every key field alone
        for f in KEY_FIELDS:
            w = dict(key)
            w[f] = (1 - key[f]) if OTHER[f] is None else OTHER[f]
            assert w[f] != key[f]
            new = s if f != "L" else s[:w["L"]]
            cases.append((key, w, s, new))
            # (another length or another circular flag is another string as well: the wrap differs)
            want_hit.append((0 if f in ("L", "circular") else 1, 0))
        # the string alone: its last byte, its first, one in the middle
        for at in (key["L"] - 1, 0, key["L"] // 2):
            t = s[:at] + ("A" if s[at] != "A" else "C") + s[at + 1:]
            cases.append((key, dict(key), s, t))
            want_hit.append((0, 0))
        # a longer new string that begins with the kept one, under a key that says so
        longer = dict(key, L=key["L"] + 1)
        cases.append((key, longer, s, s + "A"))
        want_hit.append((0, 0))
        # bytes behind the key's length do not count: the context's buffer may be longer than the string
        cases.append((key, dict(key), s + "GG", s + "TT"))
        want_hit.append((1, 1))
        assert ask_hit(driver, cases) == want_hit


def ask_route(driver, axes, cfgs):
    names = sorted(DEFAULTS)
    text = "axes %d\n" % len(axes) + "".join("%s %s\n" % (k, " ".join(str(int(v)) for v in vs)) for k, vs in axes)
    text += "cfgs %d %s\n" % (len(cfgs), " ".join(names)) + "".join(" ".join(str(int({**DEFAULTS, **c}[k])) for k in names) + "\n" for c in cfgs)
    out = subprocess.run([driver, "route"], input=text.encode(), check=True, stdout=subprocess.PIPE, timeout=300).stdout
    w = np.frombuffer(out, np.uint64).reshape(-1, 5)
    assert len(w) == len(cfgs) * int(np.prod([len(vs) for _, vs in axes]))
    return w


def test_ref_ready_sets_prep_none_with_the_band_pipeline_and_moves_nothing_else(driver):
    # the axes and switch settings of test_every_route_agrees_with_the_parents_expressions
    axes = [(b, [0, 1]) for b in BOOLS] + [("kh_entries", [0, 40]), ("plane_words", [682, 683, 1621, 1622]), ("wrap", [1 << 22, (1 << 22) + 1])]
    cfgs = switch_settings()
    checked = with_bx = 0
    for n in NS:
        for step in (0, 1):
            w = ask_route(driver, [("n", [n]), ("rejects", [n // 20 + step])] + axes, cfgs)
            assert np.array_equal(w[:, 0], w[:, 2]) and np.array_equal(w[:, 1], w[:, 3])      # every other field, and the plan's grids
            bx = unpack(w[:, 0])["bx"].astype(np.int64)
            assert not (w[:, 4] & np.uint64(1)).any()                                           # ref_ready = false: never
            assert np.array_equal((w[:, 4] >> np.uint64(1)).astype(np.int64), bx)               # ref_ready = true: exactly with bx
            checked += len(w)
            with_bx += int(bx.sum())
    assert checked == len(NS) * 2 * 256 * 2 * 4 * 2 * len(cfgs) and 0 < with_bx < checked


def test_the_steady_step_that_adopts(driver):
    # configs[1] at steady state on a hit: the reference does not come as ASCII (pend_encode = 0), so no fused launch -- and no other
    step = dict(n=1000000, flat=1, rejects=3000, deferred=1, pend_encode=0, wrap=16875, L=16619, plane_words=281)
    w = ask_route(driver, [], [step])
    r = {k: int(v[0]) for k, v in unpack(w[:, 2]).items()}
    assert int(w[0, 4]) == 2 and r["bx"] == 1 and r["fused_prep"] == 0 and r["quick"] == 1 and r["quick_phase"] == 5 and r["fork_at_quick"] == 1
