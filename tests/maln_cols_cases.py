"""The .maln files of the strand-split column table (ma_hip -f 42) that no other module makes: the smallest shapes at which k_ma_cols
can go wrong.  Rebuilt from fixed seeds on maln_synth's Maln and writer; nothing here is committed as text.

The kernel cuts the reference into tiles of T = MA_COLS_TILE columns (csrc/ma_cols_body.h, read here so that the cases move with it)
and the records into slices; a workgroup holds one tile's sixteen words per column in LDS, lists the records of its slice that have a
column or an anchor in the tile, and walks the part of each that lies in the tile.

  hand          L = 12, ACGTNACGTacg, four records: a forward one, a reverse one, the back half of a forward read, and a reverse front
                half with a lower-case letter, a '-' and an N.  Its table is written out by hand in the test.
  tile_m1, tile_0, tile_p1
                L = T-1, T, T+1: records that end on the last column (for T+1 that is a tile of one column), on both strands
  tile_edges    L = 3T+1, on both strands and with every segment (a, f, b, n): records ending on T-1, starting on T, covering T-1 .. T,
                one of 2T+2 columns (a whole tile and parts of two more), START 0 and END L-1
  outside       a forward whole record without columns at START 0 (its end is column -1), one that ends on column L on each strand
                (which the tally allows), and a record without columns at START L-1 and one in the middle
  pile_70000    70 000 identical records of three columns, two forward to one reverse, and one different record: a count that does
                not fit 16 bits.  For the library call only.
"""
import os
import re

import maln_ace_cases as mc
import maln_ends_cases as ec
import maln_synth as ms

with open(os.path.join(os.path.dirname(ms.HERE), "mapping-iterative-assembler_amd", "csrc", "ma_cols_body.h")) as _f:
    T = int(re.search(r"constexpr int MA_COLS_TILE = (\d+);", _f.read()).group(1))

CASES = ("hand", "tile_m1", "tile_0", "tile_p1", "tile_edges", "outside")
LIBRARY_ONLY = ("pile_70000",)
PILE = 70000


def _text(m, start, n, k):
    """the reference over start .. start + n - 1 with a few '-', N, lower-case letters and other bases, moved along by k"""
    seq = list(ec._ref(m, start, n))
    for c in range(n):
        q = c + k
        if q % 7 == 3:
            seq[c] = "-"
        elif q % 11 == 5:
            seq[c] = "N"
        elif q % 13 == 6:
            seq[c] = seq[c].lower()
        elif q % 5 == 1:
            seq[c] = "ACGT"[q % 4]
    return "".join(seq)


def make_hand():
    m = mc._blank("hand", 12, ms.Rng(4201), {})
    m.ref_seq = "ACGTNACGTacg"
    ec._rec(m, "fwd", 1, "CGTT")                            # columns 1 .. 4
    ec._rec(m, "rev", 3, "TNAC", rc=1, seg="a")             # columns 3 .. 6
    ec._rec(m, "back_half", 8, "TAC", seg="b")              # columns 8 .. 10: no start
    ec._rec(m, "front_half", 7, "g-NA", rc=1, seg="f")      # columns 7 .. 10: no end
    return m


def make_tile(L, name):
    rng = ms.Rng(4210 + L % 7)
    m = mc._blank(name, L, rng, {L // 2: 1})
    k = 0
    for rc in (0, 1):
        for n in (1, 2, 63, 64, 65, 130, L):               # all of them end on column L-1
            ec._rec(m, "t%d" % k, L - n, _text(m, L - n, n, k), rc=rc, seg="nafb"[k % 4], dr=int(k % 5 == 2))
            k += 1
        ec._rec(m, "z%d" % k, 0, _text(m, 0, 70, k), rc=rc)
        k += 1
    for j in range(40):
        n = int(rng.integers(1, 200, 1)[0])
        start = int(rng.integers(0, L - n + 1, 1)[0])
        ec._rec(m, "r%d" % j, start, _text(m, start, n, j), rc=j & 1, seg="nnnafb"[j % 6], dr=int(j % 9 == 4))
    return m


def make_tile_edges():
    rng = ms.Rng(4220)
    L = 3 * T + 1
    m = mc._blank("tile_edges", L, rng, {T: 1})
    k = 0
    for rc in (0, 1):
        for seg in "afbn":
            for start, n in ((T - 37, 37),                  # ends on T-1
                             (T, 41),                       # starts on T
                             (T - 1, 2),                    # covers T-1 .. T
                             (T - 3, 2 * T + 2),            # a whole tile and parts of two more
                             (0, 29),                       # START 0
                             (L - 33, 33)):                 # END L-1, the only column of the last tile
                ec._rec(m, "e%d" % k, start, _text(m, start, n, k), rc=rc, seg=seg, dr=int(k % 7 == 3))
                k += 1
    return m


def make_outside():
    rng = ms.Rng(4230)
    L = 50
    m = mc._blank("outside", L, rng, {20: 2})
    ec._rec(m, "none_at_0", 0, "")                          # e = -1
    for rc in (0, 1):
        ec._rec(m, "end_L_%d" % rc, L - 24, _text(m, L - 24, 25, rc), rc=rc)      # END = L: one column beyond, the end outside
        ec._rec(m, "none_mid_%d" % rc, 30, "", rc=rc, seg="a")                   # start on 30, end on 29
    ec._rec(m, "none_last", L - 1, "", rc=1)                # start on L-1, end on L-2
    ec._rec(m, "end_L_dropped", L - 9, _text(m, L - 9, 10, 5), dr=1)
    ec._rec(m, "end_L_front", L - 4, _text(m, L - 4, 5, 2), rc=1, seg="f")       # a column beyond, but no end event at all
    for j in range(12):
        n = 5 + 3 * j
        ec._rec(m, "o%d" % j, j, _text(m, j, n, j), rc=j & 1, seg="nafb"[j % 4])
    return m


def make_pile_70000():
    rng = ms.Rng(4240)
    m = mc._blank("pile_70000", 40, rng, {})
    at = PILE // 3 + 1
    for k in range(PILE + 1):
        if k == at:
            ec._rec(m, "other", 9, "TTg-A", rc=1)
        else:
            ec._rec(m, "p%d" % k, 10, "AC-", rc=int(k % 3 == 2))
    return m


def make_case(name):
    if name.startswith("tile_") and name != "tile_edges":
        return make_tile({"tile_m1": T - 1, "tile_0": T, "tile_p1": T + 1}[name], name)
    return {"hand": make_hand, "tile_edges": make_tile_edges, "outside": make_outside, "pile_70000": make_pile_70000}[name]()


def cutting_region(m):
    """a -R region that cuts the case: it begins and ends inside the reference and, where there is more than one tile, spans the
    first tile edge"""
    L = m.L
    if L > T + 8:
        return "%d:%d" % (T - 5, T + 8)
    return "%d:%d" % (L // 3 + 1, L - L // 4)
