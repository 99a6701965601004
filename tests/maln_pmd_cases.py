"""The .maln files of the damage score (ma_hip -L, -K, -S, -f 97; MiaHip.ma_score): every case of the deaminated-fragment filter
(tests/maln_damage_cases.py, by import) and the smallest shapes at which the kernels of csrc/mia_ma_pmd_kernels.h can go wrong.  Rebuilt
from fixed seeds on maln_synth's Maln; nothing here is committed as text.  A case is (Maln, [use masks]); every case is also run with
use = None.  own_tables(name) lists the weight tables a case brings along, beside the library's and the random one.

  edges           records of 0, 1, 15, 16, 17, 1 023 .. 1 025 and 4 095 .. 4 097 columns, each placed so that it begins, and again so that
                  it ends, on, one before and one behind a multiple of 16 (a lane's stretch), of 1 024 (a wavefront's positions) and of
                  4 096 (a workgroup's chunk); filler records in between; both strands
  span3           a record of 9 000 columns behind one of 100: it lies in three chunks
  big             a record of 5 000 columns and a pair of halves, with the tables "plus" (every entry 2^20: the score leaves int32) and
                  "minus" (every entry -2^20)
  signs           written out by hand (tests/test_ma_pmd_cpu.py) for the table "hand" (C>C -1, C>T +3, G>G -32 768, G>A 2^20 at every
                  position): S = -1, -32 768 and -32 769 (the floor division), 0, the threshold 5 exactly and 4, halves of opposite sign with
                  the sum on either side of the threshold, a pair given back half first, bins 63 and 0 (clamped and exact), an orphan, a
                  reverse record, a dropped record; the use masks switch one half of a molecule off, and both
  signs_permuted  the same records in another order
"""
import numpy as np

import maln_ace_cases as mc
import maln_damage_cases as dc
import maln_synth as ms

OWN = ("edges", "span3", "big", "signs", "signs_permuted")
CASES = dc.CASES + OWN
LANE, WAVE, CHUNK = 16, 1024, 4096                           # flat positions of a lane, a wavefront, a workgroup of k_ma_score_cols
EDGE_LENS = (0, 1, 15, 16, 17, 1023, 1024, 1025, 4095, 4096, 4097)
MAX_WEIGHT = 1 << 20
A, C, G, T = 0, 1, 2, 3
SIGNS_THRESHOLD = 5
SIGNS_IDS = ["neg1", "neg32768", "neg32769", "zero", "five", "four", "up_f", "up_b", "down_f", "down_b", "low_b", "low_f", "top", "bottom", "floor0",
             "orph_f", "rev", "drop"]


def hand_table():
    w = np.zeros((31, 5, 5), np.int32)
    w[:, C, C], w[:, C, T], w[:, G, G], w[:, G, A] = -1, 3, -32768, MAX_WEIGHT
    return w


def random_table(seed=9790):
    """adversarial: every entry, the N classes too, anywhere in -2^20 .. 2^20"""
    w = ms.Rng(seed).integers(-MAX_WEIGHT, MAX_WEIGHT + 1, 775).astype(np.int32).reshape(31, 5, 5)
    w[0, 0, 0], w[30, 4, 4] = MAX_WEIGHT, -MAX_WEIGHT
    return w


def own_tables(name):
    if name == "big":
        return [("plus", np.full((31, 5, 5), MAX_WEIGHT, np.int32)), ("minus", np.full((31, 5, 5), -MAX_WEIGHT, np.int32))]
    if name.startswith("signs"):
        return [("hand", hand_table())]
    return []


def tables(name, ds, ss):
    """every table a case is scored with: the model's two (given by the caller: the library's, or the restatement's), the random one
    and the case's own"""
    return [("ds", ds), ("ss", ss), ("random", random_table())] + own_tables(name)


def thresholds(name, mol_score):
    """0, 3 nat and the case's median score under the table at hand (the hand case: its own threshold too)"""
    median = int(np.floor(np.median(mol_score))) if len(mol_score) else 0
    return [0, 3 * 65536, median] + ([SIGNS_THRESHOLD] if name.startswith("signs") else [])


def _damaged(m, rng, start, n):
    """the reference's columns with a third of the C read as T, a third of the G as A, a few '-' and a few other bases"""
    ref = np.frombuffer(m.ref_seq[start:start + n].encode(), np.uint8)
    u = rng.random(n)
    seq = np.where((ref == ord("C")) & (u < 0.33), ord("T"), ref)
    seq = np.where((ref == ord("G")) & (u > 0.67), ord("A"), seq)
    seq = np.where((u > 0.48) & (u < 0.50), ord("-"), seq)
    seq = np.where((u > 0.50) & (u < 0.52), mc.ACGT[rng.integers(0, 4, n)], seq)
    return seq.astype(np.uint8).tobytes().decode()


def _add_damaged(m, rng, rid, n, rc):
    start = int(rng.integers(0, m.L - n + 1, 1)[0])
    return dc.add(m, rid, start, _damaged(m, rng, start, n), rc=rc)


def make_edges():
    rng = ms.Rng(9701)
    m = mc._blank("edges", 4200, rng, {})
    at, begins, ends = 0, set(), set()
    for unit in (LANE, WAVE, CHUNK):
        for n in EDGE_LENS:
            for delta in (-1, 0, 1):
                for what in ("begins", "ends"):
                    fill = (delta - at - (n if what == "ends" else 0)) % unit
                    if fill:
                        _add_damaged(m, rng, "fill%d" % len(m.rec), fill, len(m.rec) & 1)
                    at += fill
                    _add_damaged(m, rng, "%s%d_%d_%d" % (what, unit, n, delta), n, (len(m.rec) >> 1) & 1)
                    (begins if what == "begins" else ends).add((unit, n, (at if what == "begins" else at + n) % unit))
                    at += n
    for unit in (LANE, WAVE, CHUNK):
        for n in EDGE_LENS:
            for delta in (unit - 1, 0, 1):
                assert (unit, n, delta) in begins and (unit, n, delta) in ends
    return m, []


def make_span3():
    rng = ms.Rng(9702)
    m = mc._blank("span3", 9100, rng, {})
    dc.add(m, "head", 30, _damaged(m, rng, 30, 100))
    dc.add(m, "long", 50, _damaged(m, rng, 50, 9000), rc=1)
    dc.add(m, "tail", 70, _damaged(m, rng, 70, 40))
    assert 100 // CHUNK == 0 and (100 + 9000 - 1) // CHUNK == 2
    return m, []


def make_big():
    rng = ms.Rng(9703)
    L = 5100
    m = mc._blank("big", L, rng, {})
    dc.add(m, "long", 20, _damaged(m, rng, 20, 5000))
    dc.add(m, "w_f", L - 30, _damaged(m, rng, L - 30, 30), seg="f", smp=dc.smp_front(30))
    dc.add(m, "w_b", 0, _damaged(m, rng, 0, 25), seg="b", smp=dc.smp_back(25))
    dc.add(m, "short", 400, _damaged(m, rng, 400, 33), rc=1)
    n = len(m.rec)
    return m, [np.array([1, 0, 1, 1], np.uint8), np.zeros(n, np.uint8)]


def make_signs(permuted):
    m = mc._blank("signs_permuted" if permuted else "signs", 30 * len(SIGNS_IDS), ms.Rng(9704), {})
    # id -> (segment, rc, {column: reference character + SEQ character, as stored})
    specs = {"neg1": ("n", 0, {0: "CC"}), "neg32768": ("n", 0, {0: "GG"}), "neg32769": ("n", 0, {0: "GG", 1: "CC"}), "zero": ("n", 0, {}),
             "five": ("n", 0, {0: "CT", 5: "CT", 9: "CC"}), "four": ("n", 0, {0: "CT", 5: "CT", 9: "CC", 10: "CC"}),
             "up_f": ("f", 0, {0: "CT", 1: "CT"}), "up_b": ("b", 0, {3: "CC"}), "down_f": ("f", 0, {0: "CT", 1: "CT"}), "down_b": ("b", 0, {3: "CC", 4: "CC"}),
             "low_b": ("b", 0, {2: "CT"}), "low_f": ("f", 0, {0: "GG"}), "top": ("n", 0, {0: "GA", 7: "GA"}), "bottom": ("n", 0, {k: "GG" for k in range(21)}),
             "floor0": ("n", 0, {k: "GG" for k in range(20)}), "orph_f": ("f", 0, {0: "CT"}), "rev": ("n", 1, {0: "GA", 1: "GG"}), "drop": ("n", 0, {0: "CT"})}
    assert list(specs) == SIGNS_IDS
    region = {rid: k for k, rid in enumerate(sorted(SIGNS_IDS, key=lambda rid: "bnf".index(specs[rid][0])))}      # back halves lie in front of front halves
    ref = list("A" * m.L)
    for rid in SIGNS_IDS:
        seg, rc, cols = specs[rid]
        start, seq = 30 * region[rid], list("A" * 30)
        for c, pair in cols.items():
            ref[start + c], seq[c] = pair[0], pair[1]
        smp = dc.smp_front(30) if seg == "f" else dc.smp_back(30) if seg == "b" else None
        dc.add(m, rid, start, "".join(seq), rc=rc, seg=seg, smp=smp, dr=rid == "drop")
    m.ref_seq = "".join(ref)
    by_id = {rid: k for k, rid in enumerate(SIGNS_IDS)}
    masks = [np.ones(len(SIGNS_IDS), np.uint8) for _ in range(3)]
    masks[0][by_id["up_b"]] = 0                              # S of "up" becomes 6
    masks[1][by_id["down_f"]] = 0                            # S of "down" becomes -2; it still counts
    masks[2][[by_id["low_b"], by_id["low_f"]]] = 0           # "low" no longer counts
    if permuted:
        perm = ms.Rng(9705).permutation(len(m.rec)).tolist()
        m.rec = [m.rec[p] for p in perm]
        masks = [mask[perm] for mask in masks]
    return m, masks


def make_case(name):
    if name in dc.CASES:
        return dc.case(name)
    return {"edges": make_edges, "span3": make_span3, "big": make_big, "signs": lambda: make_signs(False), "signs_permuted": lambda: make_signs(True)}[name]()


_cache = {}


def case(name):
    """(Maln, [use masks])"""
    if name not in _cache:
        _cache[name] = make_case(name)
    return _cache[name]


def uses(name):
    """None and the case's masks"""
    return [None] + case(name)[1]
