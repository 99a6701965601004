"""The .maln files of the SAM export (ma_hip -f 8) that no other module makes: the smallest shapes at which the walk of
k_ma_sam_layout / k_ma_sam_render (stretches of 64 walk positions, runs carried from one stretch into the next, decimal run lengths,
an ordered scan over workgroups of 8 records) can go wrong.  Rebuilt from fixed seeds; nothing here is committed as text.

  sam_shapes   hand-placed records on a circular-looking reference of 1 500 columns:
                 walks of 1, 63, 64, 65, 127, 128, 129 and 600 positions, without an insert (walk = columns) and with one
                 ("walkNi": N - 3 columns and an insert of 3);
                 one run across a stretch edge (100M), one across three stretches (192M), an insert of 150 that begins inside
                 stretch 0 and ends in stretch 3;
                 run lengths 9, 10, 99, 100 and 1000 as M, 10, 99 and 100 as D, 9, 10, 99, 100 and 1000 as I;
                 an insert at position 0; an insert directly before and one directly after a '-' column; an insert holding '-' and
                 one of nothing else; two INS_POS pairs for one position; an insert longer than GAPS; pairs behind END and in front
                 of position 0; a record of only '-'; records without columns (one with a pair); records that end on column L with a
                 base, with '-', with an insert there, with an insert of '-' there; segments f and b on both strands; a dropped record
  sam_lower    sam_shapes with the reference in lower case (NM must not change)
  sam_257, sam_4097   257 and 4 097 short records: 32 and 512 full workgroups of the layout and one record more
  sam_empty    no records
  SCAN_EDGES   sam_8, sam_9: one workgroup of the layout, and one record more
"""
import copy

import numpy as np

import maln_ace_cases as mc
import maln_synth as ms

CASES = ("sam_shapes", "sam_lower", "sam_257", "sam_4097", "sam_empty")
SCAN_EDGES = ("sam_8", "sam_9")
L_SHAPES = 1500


def _rec(m, rid, start, seq, ins=(), rc=0, seg="n", dr=0, tr=0, num_inputs=1):
    n = len(seq)
    m.rec.append({"id": rid, "desc": "", "score": 900 + 17 * len(m.rec), "num_inputs": num_inputs, "start": start, "end": start + n - 1, "rc": rc, "tr": tr,
                  "dr": dr, "seg": seg, "seq": seq, "smp": mc._smp(n), "ins": list(ins)})


def _ref(m, start, n):
    """the reference's own characters: a record of matches (column L reads as column 0)"""
    return "".join(m.ref_seq[(start + k) % m.L] for k in range(n))


def make_shapes():
    rng = ms.Rng(8001)
    L = L_SHAPES
    m = mc._blank("sam_shapes", L, rng, {40: 2, 300: 3, 700: 1})
    for k, w in enumerate((1, 63, 64, 65, 127, 128, 129, 600)):
        mc._record(m, rng, "walk%d" % w, 10 + 31 * k, w, rc=k & 1, seg="nfba"[k % 4])
        mc._record(m, rng, "walk%di" % w, 700 + 13 * k, max(w - 3, 1), ins=[(max(w - 3, 1) // 2, mc._bases(rng, 3))] if w > 3 else [])
    _rec(m, "run100M", 200, _ref(m, 200, 100))
    _rec(m, "run192M", 260, _ref(m, 260, 192), rc=1)
    _rec(m, "ins150", 50, _ref(m, 50, 230), ins=[(50, mc._bases(rng, 150))])
    digits = _ref(m, 100, 9) + "-" + _ref(m, 110, 10) + "-" * 10 + _ref(m, 130, 99) + "-" * 99 + _ref(m, 328, 100) + "-" * 100 + _ref(m, 528, 900)
    _rec(m, "digitsM_D", 100, _ref(m, 100, 1000) + "-" + _ref(m, 1101, 5))                                    # 1000M1D5M
    _rec(m, "digitsMD", 100, digits, seg="f")                                                                    # 9M1D10M10D99M99D100M100D900M
    _rec(m, "digitsI", 20, _ref(m, 20, 12), ins=[(1, mc._bases(rng, 9)), (3, mc._bases(rng, 10)), (5, mc._bases(rng, 99)), (7, mc._bases(rng, 100)),
                                                 (9, mc._bases(rng, 1000))], rc=1, seg="b")
    _rec(m, "ins_at_0", 300, _ref(m, 300, 30), ins=[(0, "ACG")])
    _rec(m, "ins_by_dash", 310, _ref(m, 310, 3) + "-" + _ref(m, 314, 4), ins=[(3, "TT"), (4, "G")])             # 3M2I1D1I4M
    _rec(m, "ins_with_dash", 320, _ref(m, 320, 20), ins=[(5, "A-C"), (9, "--"), (12, "-T-")])
    _rec(m, "ins_twice", 330, _ref(m, 330, 20), ins=[(6, "GGGG"), (6, "A"), (10, "C"), (10, "--"), (14, "-"), (14, "TTT")])
    _rec(m, "ins_over_gaps", 290, _ref(m, 290, 20), ins=[(10, "ACGTA")])                                         # GAPS[300] = 3
    _rec(m, "ins_outside", 340, _ref(m, 340, 10), ins=[(10, "AAA"), (12, "C"), (-1, "GG"), (4, "T")])
    _rec(m, "only_dashes", 400, "-" * 70)
    _rec(m, "no_columns", 410, "")
    _rec(m, "no_columns_pair", 411, "", ins=[(0, "ACGT")])
    for k, (seg, rc) in enumerate((("f", 0), ("f", 1), ("b", 0), ("b", 1))):
        mc._record(m, rng, "seg_%s%d" % (seg, rc), 420 + k, 40, rc=rc, seg=seg)
    mc._record(m, rng, "dropped", 430, 35, dr=1, tr=1, num_inputs=4)
    mc._record(m, rng, "dropped_b_rc", 431, 35, dr=1, rc=1, seg="b")
    # records of a circular assembly that end on column L
    _rec(m, "end_L", L - 30, _ref(m, L - 30, 31), seg="f")
    _rec(m, "end_L_dash", L - 29, _ref(m, L - 29, 29) + "-", seg="f", rc=1)
    _rec(m, "end_L_ins", L - 28, _ref(m, L - 28, 29), ins=[(28, "ACG"), (27, "T")], seg="f")
    _rec(m, "end_L_ins_dash", L - 27, _ref(m, L - 27, 27) + "-", ins=[(27, "--")], seg="f")
    _rec(m, "end_Lm1", L - 64, _ref(m, L - 64, 64))
    return m


def make_lower():
    m = make_shapes()
    m.ref_id = "sam_lower"
    m.ref_seq = m.ref_seq.lower()
    return m


def make_many(n, seed):
    rng = ms.Rng(seed)
    L = 900
    m = mc._blank("sam_%d" % n, L, rng, {450: 2})
    length = rng.integers(1, 40, n)
    start = rng.integers(0, L - 40, n)
    has = rng.random(n) < 0.3
    for i in range(n):
        k = int(length[i])
        ins = [(int(k // 2), mc._bases(rng, 1 + i % 3))] if has[i] else []
        mc._record(m, rng, "q%d" % i, int(start[i]), k, rc=i & 1, seg="nfb"[i % 3], ins=ins, dr=int(i % 7 == 0), dash=0.08)
    return m


def make_case(name):
    if name == "sam_shapes":
        return make_shapes()
    if name == "sam_lower":
        return make_lower()
    if name == "sam_empty":
        m = mc.make_empty()
        m.ref_id = "sam_empty"
        return m
    return make_many(int(name[4:]), 8100 + int(name[4:]))


def case_text(name):
    """the .maln from its MALN_NAS line on"""
    return ms.write_maln(make_case(name))


def negative_gap(m):
    bad = copy.copy(m)
    bad.gaps = m.gaps.copy()
    bad.gaps[m.L // 2] = -1
    return bad
