"""The lean quick plan (csrc/bandx_body.h: bx_quick and bx_quick2 with one seek per read, the N credit compiled out, block tests by
clean-run masks) against the forms it replaces, frozen in
tests/emul/bandx_quick_parent.h: the same BxPlan, field by field (mode, d0, w, b0, dstar, edge), and the same refusals, for

  * EVERY diagonal of every window (and the two just outside it) -- a superset of the diagonals with few mismatches that
    tests/test_emul_bandx.py asks the quick plan about --, over that file's kinds of queries: damaged reads with substitutions, single
    indels anywhere, two indels, wrapped references (tandem duplications included), references with a handful of N columns;
  * reads of 36 .. 256 bases under every NW (64-row words of the run's longest read) the kernel could run them with, NW = 1 .. 4;
  * the flat, ancient and solexa matrices, both strands;
  * the one-indel form asked three ways: the frozen one, the lean one on a fresh scan (the kernel), the lean one on the scan the first form
    left behind (bx_plan_quick).

No query is skipped: the driver returns how many it asked and how many answers differed.

Handing the bitmaps' answers (the blocks' `uniq` / `absent` masks) on from the first form to the second was NOT built, so there are no carried
masks to check against recomputed ones: `looked_up` below counts the reads it could have served -- planned by the one-indel form after the
one-diagonal form had asked the bitmaps about them -- and finds a handful among hundreds (a read that is clean for ten rows on another
diagonal loses most of those rows on d, and with more than BX_QUICK_MAX lost rows the first form never asks)."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_emul_align import codes
from test_emul_bandx import MATS, damage, pssm_pair, window
from test_emul_diag_filter import mutate


@pytest.fixture(scope="module")
def lean(oracle_build):
    out = os.path.join(oracle_build, "libmia_quick_lean.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", "mapping-iterative-assembler_amd/csrc", "-I", "tests/emul", "-o", out,
                    "tests/emul/emu_quick_lean.cpp"], cwd=ROOT, check=True)
    lib = C.CDLL(out)
    lib.ql_tab_new.restype = C.c_void_p
    lib.ql_ref_new.restype = C.c_void_p
    lib.ql_compare.restype = C.c_int
    lib.ql_tab_ok.restype = C.c_int
    return lib


class Tables:
    def __init__(self, lean, oracle, spec):
        fwd, rc = pssm_pair(oracle, spec)
        self.lean = lean
        self.h = C.c_void_p(lean.ql_tab_new(fwd.ctypes.data_as(C.c_void_p), rc.ctypes.data_as(C.c_void_p)))
        assert lean.ql_tab_ok(self.h) == 1, spec

    def close(self):
        self.lean.ql_tab_free(self.h)


class Ref:
    def __init__(self, lean, ref, wrapped=False):
        self.lean, self.ref = lean, ref
        rc = codes(ref)
        self.h = C.c_void_p(lean.ql_ref_new(rc.ctypes.data_as(C.c_void_p), C.c_int64(len(ref)), 1 if wrapped else 0))

    def close(self):
        self.lean.ql_ref_free(self.h)


KINDS = {1: "one-diagonal form", 2: "one-indel form, fresh scan", 3: "one-indel form, the first form's scan"}


def compare(lean, tab, ref, s, l1, read, strand, counts):
    c2 = codes(read)
    diff = (C.c_int32 * 32)()
    bad = lean.ql_compare(ref.h, tab.h, s, l1, c2.ctypes.data_as(C.c_void_p), len(read), strand, counts.ctypes.data_as(C.c_void_p), diff)
    v = list(diff)[:16]
    assert bad == 0, (bad, KINDS.get(v[0], v[0]), "NW", v[1], "d", v[2], "frozen (ok, mode, d0, w, b0, dstar, edge)", v[3:10], "lean (ok, mode, d0, w, b0, dstar)", v[10:16],
                      ref.ref[s:s + l1], read, strand)


def indel(rnd, read, i):
    at = rnd.randint(5, len(read) - 5)
    k = rnd.choice([1, 1, 1, 2, 3, 4])          # (up to BX_QUICK_SHIFT and one beyond it)
    return read[:at] + read[at + k:] if i % 2 else read[:at] + "".join(rnd.choice("ACGT") for _ in range(k)) + read[at:]


def read_length(rnd, i):
    # 36 .. 256 bases: below 30 the plan takes no read, 64 / 128 / 192 are where NW steps
    return [100, 100, rnd.randint(36, 64), rnd.randint(65, 128), rnd.randint(129, 192), rnd.randint(193, 256), 64, 65, 128, 129, 192, 193, 256, 36][i % 14]


@pytest.mark.parametrize("spec", ["flat", "ancient.submat.txt", "ancient.submat.solexa.pe.txt"])
def test_lean_quick_plan_gives_the_frozen_plans(lean, oracle, spec):
    rnd = random.Random(7006 + len(spec))
    tab = Tables(lean, oracle, spec)
    counts = np.zeros(8, dtype=np.int64)
    strands = [0] if spec == "flat" else [0, 1]
    assert (spec, 0) in MATS and (spec, strands[-1]) in MATS
    # plain references: substitutions, damage, one indel, two indels, clipped windows
    plain = Ref(lean, "".join(rnd.choice("ACGT") for _ in range(5000)))
    low = "".join(rnd.choice("ACGT") for _ in range(1500))
    low = low[:400] + "ACACACACAT" * 12 + low[520:900] + low[300:420] + low[1020:]          # a microsatellite and a second copy: repeated 10-mers
    lowc = Ref(lean, low)
    for i in range(420):
        ref = lowc if i % 6 == 5 else plain
        n = read_length(rnd, i)
        pos = rnd.randint(0, len(ref.ref) - n)
        read = ref.ref[pos:pos + n]
        if spec != "flat":
            read = damage(rnd, read, p0=0.6)
        read = mutate(rnd, read, rnd.sample(range(n), rnd.choice([0, 0, 1, 1, 2, 3, 4, 6, 9])))
        if i % 3 == 1:
            read = indel(rnd, read, i)
        if i % 9 == 4:
            read = indel(rnd, indel(rnd, read, i), i + 1)
        s, l1 = window(ref.ref, pos + rnd.randint(-3, 3) if 3 <= pos < len(ref.ref) - n - 3 else pos, len(read), margin=rnd.choice([50, 50, 12, 3]))
        if l1 < len(read):
            continue
        compare(lean, tab, ref, s, l1, read, strands[i % len(strands)], counts)
    plain.close()
    lowc.close()
    # wrapped references, many reads over the origin, a tandem duplication in every fifth
    for i in range(120):
        L = rnd.choice([300, 420, 700, 1500, 3000])
        core = "".join(rnd.choice("ACGT") for _ in range(L))
        if i % 5 == 0:
            a = rnd.randint(0, L - 80)
            core = core[:a + 40] + core[a:a + 40] + core[a + 80:]
        text = core + core[:256]
        n = min(read_length(rnd, i), 250)
        pos = rnd.choice([L - rnd.randint(1, n), L - n - rnd.randint(0, 40), rnd.randint(0, L - 1), rnd.randint(0, 50)])
        read = text[pos:pos + n]
        if len(read) < n:
            continue
        if i % 3 == 0:
            read = indel(rnd, read, i)
        read = damage(rnd, read) if spec != "flat" else read
        read = mutate(rnd, read, rnd.sample(range(len(read)), rnd.choice([0, 0, 1, 2, 4])))
        s, l1 = window(text, pos, len(read), margin=rnd.choice([50, 50, 120]))
        if l1 < len(read) or l1 > 760:
            continue
        ref = Ref(lean, text, wrapped=True)
        compare(lean, tab, ref, s, l1, read, strands[i % len(strands)], counts)
        ref.close()
    # references with a handful of N columns: the table spells them out, the quick plan answers for the windows that hold none
    for i in range(120):
        L = rnd.choice([1200, 2000, 4000])
        core = [rnd.choice("ACGT") for _ in range(L)]
        a = rnd.randint(100, L // 2 - 200)
        b = rnd.randint(L // 2 + 100, L - 300)
        if i % 2 == 0:
            core[b:b + 120] = core[a:a + 120]
            core[b + rnd.randint(20, 100)] = "N"
        for _ in range(rnd.choice([1, 2, 4])):
            core[rnd.randint(0, L - 1)] = rnd.choice("NNRY")
        text = "".join(core)
        n = read_length(rnd, i)
        pos = rnd.choice([a + rnd.randint(-30, 60), b + rnd.randint(-30, 60), rnd.randint(0, L - n)])
        pos = max(0, min(L - n, pos))
        read = "".join(c if c in "ACGT" else rnd.choice("ACGT") for c in text[pos:pos + n])
        if i % 3 == 0:
            read = indel(rnd, read, i)
        read = damage(rnd, read) if spec != "flat" else read
        read = mutate(rnd, read, rnd.sample(range(len(read)), rnd.choice([0, 0, 1, 2, 4])))
        s, l1 = window(text, pos, len(read), margin=rnd.choice([20, 50, 50]))
        if l1 < len(read):
            continue
        ref = Ref(lean, text)
        compare(lean, tab, ref, s, l1, read, strands[i % len(strands)], counts)
        ref.close()
    tab.close()
    asked, quick1, quick2, looked_up, _, done, values, trace = (int(x) for x in counts)
    print("lean quick plan", spec, dict(asked=asked, quick1=quick1, quick2=quick2, looked_up=looked_up, done=done, values=values, trace=trace))
    # (every query compared, three ways; the counts say the comparison was not of refusals alone)
    assert asked > 40000 and quick1 > 400 and quick2 > 100 and done > 100 and values > 100 and trace > 100, \
        "%d queries asked and compared, none skipped: %s" % (asked, list(counts))
