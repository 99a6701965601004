"""The .maln files of the fragment-end context (ma_hip -f 92) and the read lengths (-f 93) that no other module makes: the smallest
shapes at which k_ma_ends can go wrong.  Rebuilt from fixed seeds on maln_synth's Maln and writer; nothing here is committed as text.

The kernel takes a record per lane, 64 per wavefront, 256 per workgroup (csrc/mia_ma_ends_kernels.h), reads the record's columns in
16-byte words from the word that holds its first column to the word that holds its last (csrc/ma_ends_body.h), and adds every event to
the wavefront's copy of the bins in LDS.

  hand12        L = 12, ACGTNACGTacg, three records: a forward one with a '-' and an insert that holds a '-', a reverse one with two
                pairs for position 0, and the back half of a forward read.  Its tables are written out by hand in the test.
  short_ref     L = 7: every window leaves the reference on both sides
  edges         L = 600: records with START = 0 .. 10 and records with END = L-11 .. L-1, each on both strands and with every
                segment (a, f, b, n); one that ends on column L (which the tally allows; the file's GAPS sum is 2 -- the reference's
                format 3 reads past its arrays for such a record in a file without a gap); one without columns at START 450
  codes         N, the other IUPAC letters and lower case in the reference, under and around the ends, both strands, all segments
  pile_<K>      K = 63, 64, 65, 255, 256, 257 identical records and one different: the edges of a wavefront and of a workgroup, and
                every lane of a wavefront on the same 41 bins
  pile_5000     5 000 records in a few piles, every third marked DR: more than one workgroup, bins far above 16 bits' worth of lanes
  lens          whole records of length 0 (all '-'), 1, 255, 256 and, with inserts, 511, 512, 513 and 700; two pairs for one position;
                pairs at n-1, n and -1; a '-' inside an insert; START at every residue of 16 (the first word's mask) and n around 16
                and 32; both strands; halves that must not count
"""
import maln_ace_cases as mc
import maln_synth as ms

PILES = (63, 64, 65, 255, 256, 257)
CASES = ("hand12", "short_ref", "edges", "codes") + tuple("pile_%d" % k for k in PILES) + ("pile_5000", "lens")
LENS_WANTED = (0, 1, 255, 256, 511, 512, 513, 700)
IUPAC = "NnRYKMSWBDHVrykmswbdhvXx."


def _rec(m, rid, start, seq, rc=0, seg="n", ins=(), dr=0):
    n = len(seq)
    m.rec.append({"id": rid, "desc": "", "score": 700 + 11 * len(m.rec), "num_inputs": 1, "start": start, "end": start + n - 1, "rc": rc, "tr": 0,
                  "dr": dr, "seg": seg, "seq": seq, "smp": mc._smp(n), "ins": list(ins)})
    for pos, text in ins:                                  # GAPS wide enough for every insert that counts
        if 0 <= pos < n and start + pos < m.L:
            m.gaps[start + pos] = max(int(m.gaps[start + pos]), len(text))


def _ref(m, start, n):
    return (m.ref_seq + "ACGT" * (n // 4 + 1))[start:start + n].upper().translate(str.maketrans(IUPAC, "A" * len(IUPAC)))


def make_hand12():
    m = mc._blank("hand12", 12, ms.Rng(9201), {})
    m.ref_seq = "ACGTNACGTacg"
    _rec(m, "fwd", 2, "GT-AC", ins=[(1, "A-C")])                                   # columns 2 .. 6: length 4 + 2
    _rec(m, "rev", 5, "ACGT", rc=1, ins=[(0, "GG"), (0, "T")])                     # columns 5 .. 8: the later pair counts, length 4 + 1
    _rec(m, "back_half", 9, "ACG", seg="b")                                        # columns 9 .. 11: a 3' end only, no length
    return m


def make_short_ref():
    rng = ms.Rng(9202)
    m = mc._blank("short_ref", 7, rng, {3: 1})
    k = 0
    for start, n in ((0, 7), (0, 1), (6, 1), (2, 3), (3, 0), (1, 6)):
        for rc in (0, 1):
            _rec(m, "s%d" % k, start, _ref(m, start, n), rc=rc, seg="anfb"[k % 4], dr=int(k == 5))
            k += 1
    return m


def make_edges():
    rng = ms.Rng(9203)
    L = 600
    m = mc._blank("edges", L, rng, {300: 2})
    k = 0
    for rc in (0, 1):
        for seg in "afbn":
            for i in range(11):
                n = 30 + (7 * k) % 40
                mc._record(m, rng, "s%d" % k, i, n, rc=rc, seg=seg, dr=int(k % 13 == 5))
                mc._record(m, rng, "e%d" % k, L - 11 + i - n + 1, n, rc=rc, seg=seg)
                k += 1
    for rc in (0, 1):
        _rec(m, "end_L_%d" % rc, L - 24, _ref(m, L - 24, 25), rc=rc)               # END = L
    mc._record(m, rng, "no_columns", 450, 0, dash=0.0)
    _rec(m, "no_columns_rc", 450, "", rc=1, seg="a")
    return m


def make_codes():
    rng = ms.Rng(9204)
    L = 200
    m = mc._blank("codes", L, rng, {100: 1})
    pool = "ACGTacgt" + IUPAC
    m.ref_seq = "".join(pool[int(x)] for x in rng.integers(0, len(pool), L))
    for k in range(80):
        n = int(rng.integers(1, 60, 1)[0])
        start = int(rng.integers(0, L - n + 1, 1)[0])
        _rec(m, "c%d" % k, start, _ref(m, start, n), rc=k & 1, seg="nnafbn"[k % 6], dr=int(k % 11 == 3))
    return m


def make_pile(K):
    rng = ms.Rng(9300 + K)
    L = 400
    m = mc._blank("pile_%d" % K, L, rng, {200: 1})
    seq = _ref(m, 120, 61)
    seq = seq[:20] + "-" + seq[21:]
    at = K // 3
    for k in range(K + 1):
        if k == at:                                        # the one that differs, somewhere inside the pile
            _rec(m, "other", 3, _ref(m, 3, 45), rc=1, ins=[(7, "AC")])
        else:
            _rec(m, "p%d" % k, 120, seq, ins=[(30, "G")])
    return m


def make_pile_5000():
    rng = ms.Rng(9305)
    L = 2000
    m = mc._blank("pile_5000", L, rng, {1000: 1})
    spots = [(int(rng.integers(0, L - 150, 1)[0]), int(rng.integers(20, 150, 1)[0]), j & 1, "nnnnafb"[j % 7]) for j in range(9)]
    texts = [_ref(m, s, n) for s, n, _, _ in spots]
    pick = rng.integers(0, 3, 5000)                        # three piles take most records, the other six the rest
    for k in range(5000):
        j = int(pick[k]) if k % 10 else 3 + (k // 10) % 6
        s, n, rc, seg = spots[j]
        _rec(m, "q%d" % k, s, texts[j], rc=rc, seg=seg, dr=int(k % 3 == 1))
    return m


def make_lens():
    rng = ms.Rng(9206)
    L = 900
    m = mc._blank("lens", L, rng, {})
    k = 0

    def rec(start, seq, **kw):
        nonlocal k
        _rec(m, "l%d" % k, start, seq, **kw)
        k += 1

    for rc in (0, 1):
        rec(100, "-" * 40, rc=rc)                                                   # length 0
        rec(101 + rc, "-" * 17 + "A" + "-" * 9, rc=rc)                              # 1
        rec(110, _ref(m, 110, 255), rc=rc)                                          # 255
        rec(111, _ref(m, 111, 256), rc=rc)                                          # 256
        rec(120, _ref(m, 120, 255), rc=rc, ins=[(100, mc._bases(rng, 256))])        # 511
        rec(121, _ref(m, 121, 256), rc=rc, ins=[(0, mc._bases(rng, 256))])          # 512
        rec(122, _ref(m, 122, 256), rc=rc, ins=[(255, mc._bases(rng, 257))])        # 513: a pair at n - 1
        rec(123, _ref(m, 123, 256), rc=rc, ins=[(10, mc._bases(rng, 300)), (200, mc._bases(rng, 144))])      # 700
        rec(300, _ref(m, 300, 50), rc=rc, ins=[(5, "ACGT"), (20, "T"), (5, "G")])   # two pairs for position 5: 50 + 1 + 1
        rec(310, _ref(m, 310, 50), rc=rc, ins=[(49, "AA"), (50, "CCC"), (-1, "GGGG")])                      # n - 1 counts; n and -1 do not: 52
        rec(320, _ref(m, 320, 50), rc=rc, ins=[(7, "A-C-"), (8, "--")])             # '-' inside an insert: 52
        rec(330, _ref(m, 330, 60), rc=rc, seg="f", ins=[(3, "AC")])                 # halves: no length
        rec(331, _ref(m, 331, 60), rc=rc, seg="b")
        rec(332, _ref(m, 332, 60), rc=rc, seg="a")
    for r16 in range(16):                                  # the flat offset of a record's first column at every residue of 16
        for n in (1, 15, 16, 17, 31, 32, 33):
            seq = list(_ref(m, 400 + r16, n))
            for c in (0, n - 1, n // 2):
                if (c + r16) % 3 == 0:
                    seq[c] = "-"
            rec(400 + r16, "".join(seq), rc=(r16 + n) & 1)
        rec(500, _ref(m, 500, 16 - r16 if r16 else 3), rc=r16 & 1)                  # shifts what follows by another residue
    return m


def make_case(name):
    if name.startswith("pile_") and name != "pile_5000":
        return make_pile(int(name[5:]))
    return {"hand12": make_hand12, "short_ref": make_short_ref, "edges": make_edges, "codes": make_codes, "pile_5000": make_pile_5000, "lens": make_lens}[name]()


def for_the_reference(m):
    """the case as the reference's `ma` may read it: read_ma stores a pair at ins[position] (src/map_alignment.c:602-605), so a pair
    with a negative position is a stray write there.  True ends do not look at INS_POS pairs."""
    import copy
    t = copy.copy(m)
    t.rec = [dict(r, ins=[(p, s) for p, s in r["ins"] if p >= 0]) for r in m.rec]
    return t
