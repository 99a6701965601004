"""The .maln files of the deaminated-fragment filter (ma_hip -D, -e, -S, -f 95; MiaHip.ma_damage): the smallest shapes at which the
kernels of csrc/mia_ma_damage_kernels.h can go wrong.  Rebuilt from fixed seeds on maln_synth's Maln and writer; nothing here is
committed as text.  A case is (Maln, [use masks]); every case is also run with use = None.

  hand            thirteen records on a reference of CGCG..: hits at k = 1, 3 and 15, a would-be hit at MIDDLE, a C>T at the 3' end
                  (a hit only for a single-stranded library), a reverse record, a pair with the hit in the front half, a pair given
                  back half first with the hit in the back half, an orphan, a dropped record.  Results are written out by hand in the
                  CPU test
  empty           no record (no launch)
  lens            records of 0, 1, 15, 16, 17 and 31 columns, either strand, every C and G of the read deaminated
  offsets         300 records of 1 .. 40 columns: a record begins and ends on every offset of a 16-position word
  edge_before, edge_behind
                  a record of 31 columns over flat positions 4 090 .. 4 120 (the chunk of a workgroup ends at 4 095) with its only hit
                  at flat 4 093 / at flat 4 100
  mirror          forward and reverse records that hold the same read: MIRROR_PAIRS lists them, they must get the same positions
                  (reads of 30 bases and more: a shorter record's bases near its last column carry 5' codes on either strand)
  odd             a C>T under a '-' column, lower-case SEQ, lower-case reference, reference N, a column at p >= L, a bad depth code on
                  a '-' column, a read shorter than 31 whose bases near the 3' end carry 5' codes
  wrap            pairs across the origin with the hit in the front half only, in the back half only, in both; orphans; halves on
                  different strands; the use masks silence the only hit of a molecule and all records of a molecule
  pile_3000       3 000 equal records: one bin of hist
  mixed           2 000 reads with simulated damage, both strands, '-' columns, 60 pairs across the origin, dropped records
  mixed_reversed  the same records in reversed order
"""
import numpy as np

import maln_ace_cases as mc
import maln_synth as ms

CASES = ("hand", "empty", "lens", "offsets", "edge_before", "edge_behind", "mirror", "odd", "wrap", "pile_3000", "mixed", "mixed_reversed")
MIRROR_PAIRS = []                                            # (forward record, reverse record) of case "mirror"
CHUNK = 4096                                                 # flat positions of a workgroup of k_ma_damage_hits
_COMP = str.maketrans("ACGTacgt", "TGCAtgca")


def revcomp(s):
    return s.translate(_COMP)[::-1]


def smp_front(n):
    """the first n codes of a long read: 1 .. 15 from the 5' end, then MIDDLE"""
    return "".join(chr(ord("A") + min(k, 15)) for k in range(n))


def smp_back(n):
    """the last n codes of a long read"""
    return "".join(chr(ord("A") + (30 - (n - 1 - k) if n - 1 - k < 15 else 15)) for k in range(n))


def add(m, rid, start, seq, rc=0, seg="n", smp=None, dr=0, score=100):
    """a record over columns start .. start + len(seq) - 1 with SEQ as given (stored orientation)"""
    n = len(seq)
    m.rec.append({"id": rid, "desc": "", "score": score, "num_inputs": 1, "start": int(start), "end": int(start) + n - 1, "rc": int(rc), "tr": 0, "dr": int(dr),
                  "seg": seg, "seq": seq, "smp": mc._smp(n) if smp is None else smp, "ins": []})
    return len(m.rec) - 1


def ref_at(m, start, n):
    return m.ref_seq[start:start + n]


def mutated(s, changes):
    t = list(s)
    for k, ch in changes.items():
        t[k] = ch
    return "".join(t)


def deaminate(read, rng, p_end=0.5, p_mid=0.02, ss=False):
    """a read (its own orientation) with C>T near its 5' end and G>A (ss: C>T) near its 3' end"""
    n = len(read)
    u = rng.random(n)
    out = list(read)
    for k in range(n):
        p5 = p_end * 0.6 ** k + p_mid
        p3 = p_end * 0.6 ** (n - 1 - k) + p_mid
        if read[k] == "C" and u[k] < p5:
            out[k] = "T"
        elif read[k] == ("C" if ss else "G") and u[k] > 1.0 - p3:
            out[k] = "T" if ss else "A"
    return "".join(out)


def make_hand():
    m = mc._blank("hand", 200, ms.Rng(9501), {})
    m.ref_seq = "CG" * 100                                   # column p is C where p is even
    r40, f20, b20 = ref_at(m, 0, 40), ref_at(m, 180, 20), ref_at(m, 0, 20)
    add(m, "h0", 0, mutated(r40, {0: "T"}))
    add(m, "h1", 0, mutated(r40, {2: "T"}))
    add(m, "h2", 0, mutated(r40, {14: "T", 39: "A"}))
    add(m, "h3", 0, mutated(r40, {38: "T"}))
    add(m, "h4", 0, mutated(r40, {16: "T"}))
    add(m, "h5", 0, mutated(r40, {39: "A", 2: "T"}), rc=1)
    add(m, "h6", 0, r40)
    add(m, "w_f", 180, mutated(f20, {2: "T"}), seg="f", smp=smp_front(20))
    add(m, "w_b", 0, b20, seg="b", smp=smp_back(20))
    add(m, "x_b", 0, mutated(b20, {19: "A"}), seg="b", smp=smp_back(20))
    add(m, "x_f", 180, f20, seg="f", smp=smp_front(20))
    add(m, "o_f", 180, mutated(f20, {0: "T"}), seg="f", smp=smp_front(20))
    add(m, "d0", 0, mutated(r40, {0: "T"}), dr=1)
    return m, []


def make_empty():
    return mc._blank("empty", 120, ms.Rng(9502), {}), []


def _all_damaged(m, start, n, rc):
    """the reference's columns with every C of the read read as T and every G as A"""
    s = ref_at(m, start, n)
    return s.translate(str.maketrans("CG", "TA")) if not rc else s.translate(str.maketrans("GC", "AT"))


def make_lens():
    rng = ms.Rng(9503)
    m = mc._blank("lens", 300, rng, {})
    for n in (0, 1, 15, 16, 17, 31, 0, 30, 32):
        for rc in (0, 1):
            for start in (5, 120):
                add(m, "l%d_%d_%d" % (n, rc, start), start, _all_damaged(m, start, n, rc), rc=rc)
    return m, []


def make_offsets():
    rng = ms.Rng(9504)
    m = mc._blank("offsets", 500, rng, {})
    lens, starts, rcs = rng.integers(1, 41, 300), rng.integers(0, 450, 300), rng.integers(0, 2, 300)
    at, begins, ends = 0, set(), set()
    for k in range(300):
        n, rc = int(lens[k]), int(rcs[k])
        read = ref_at(m, int(starts[k]), n)
        read = revcomp(deaminate(revcomp(read), rng, 0.9)) if rc else deaminate(read, rng, 0.9)
        add(m, "o%d" % k, int(starts[k]), read, rc=rc)
        begins.add(at % 16)
        ends.add((at + n - 1) % 16)
        at += n
    assert len(begins) == 16 and len(ends) == 16
    return m, []


def make_edge(behind):
    rng = ms.Rng(9505)
    m = mc._blank("edge_behind" if behind else "edge_before", 400, rng, {})
    plain = ref_at(m, 50, 10)
    for k in range(409):                                     # 4 090 flat positions without a hit
        add(m, "p%d" % k, 50, plain, rc=k & 1)
    ref = list(m.ref_seq)
    ref[100:131] = list("A" * 31)                            # no C, no G: nothing but the planted hit
    ref[100 + (10 if behind else 3)] = "C"
    m.ref_seq = "".join(ref)
    at = 10 if behind else 3                                 # flat 4 100 (k = 11) / flat 4 093 (k = 4)
    add(m, "straddle", 100, mutated(ref_at(m, 100, 31), {at: "T"}))
    for k in range(20):
        add(m, "q%d" % k, 50, plain, rc=k & 1)
    assert sum(len(r["seq"]) for r in m.rec[:409]) == CHUNK - 6
    return m, []


def make_mirror():
    rng = ms.Rng(9506)
    L = 1200
    m = mc._blank("mirror", L, rng, {})
    ref = list(m.ref_seq)
    del MIRROR_PAIRS[:]
    for k in range(12):
        n = (30, 31, 32, 33, 40, 47, 48, 45, 49, 35, 36, 31)[k]      # (from 30 columns on the codes of a record read backwards are the mirrored codes)
        a, b = 50 * k, 600 + 50 * k
        ref[b:b + n] = list(revcomp("".join(ref[a:a + n])))  # the columns at b read backwards are the columns at a
        m.ref_seq = "".join(ref)
        read = deaminate(ref_at(m, a, n), rng, 0.8, 0.1)
        MIRROR_PAIRS.append((add(m, "f%d" % k, a, read), add(m, "r%d" % k, b, revcomp(read), rc=1)))
    return m, []


def make_odd():
    m = mc._blank("odd", 100, ms.Rng(9507), {})
    ref = list("A" * 100)
    for p in (0, 1, 2, 3, 4, 40, 41):
        ref[p] = "C"
    ref[2] = "c"
    ref[3] = "N"
    ref[99] = "G"
    m.ref_seq = "".join(ref)
    base = ref_at(m, 0, 40)
    add(m, "dash", 0, mutated(base, {0: "-"}))                           # C under '-': no hit
    add(m, "lower_seq", 0, mutated(base, {1: "t"}))                      # k = 2
    add(m, "lower_ref", 0, mutated(base, {2: "T"}))                      # k = 3
    add(m, "ref_n", 0, mutated(base, {3: "T"}))                          # N>T: no hit
    add(m, "beyond", 70, ref_at(m, 70, 30) + "A")                        # its last column is p = L: would be G>A at k = 1
    add(m, "last_col", 70, mutated(ref_at(m, 70, 30), {29: "A"}))        # ... and on column L - 1 it is one
    bad = mc._smp(40)
    add(m, "bad_code", 0, mutated(base, {0: "-", 4: "T"}), smp="`" + bad[1:])      # a bad depth code on a '-' column; k = 5 still counts
    add(m, "short", 30, mutated(ref_at(m, 30, 20), {10: "T", 11: "T"}))  # 20 columns: columns 40 and 41 are positions 11 and 12 from the 5' end
    return m, []


def make_wrap():
    rng = ms.Rng(9508)
    L = 300
    m = mc._blank("wrap", L, rng, {})
    ref = list(m.ref_seq)
    ref[280], ref[282], ref[19], ref[17] = "C", "C", "G", "G"
    m.ref_seq = "".join(ref)
    front, back = ref_at(m, 280, 20), ref_at(m, 0, 20)
    swap = str.maketrans("CG", "GC")
    front, back = front.translate(swap), back.translate(swap)            # (C>G and G>C: mismatches, never hits)
    front_hit, back_hit = mutated(front, {0: "T"}), mutated(back, {19: "A"})
    front_c, back_g = mutated(front, {0: "C", 2: "C"}), mutated(back, {19: "G", 17: "G"})
    for tag, f, b in (("front", front_hit, back_g), ("back", front_c, back_hit), ("both", mutated(front_c, {2: "T"}), mutated(back_g, {17: "A"})), ("none", front_c, back_g)):
        for rc in (0, 1):
            # a reverse record's 5' end is its last column: for rc the stored strings are the same columns, the ends swap
            add(m, "%s%d_f" % (tag, rc), 280, f, rc=rc, seg="f", smp=smp_front(20))
            add(m, "%s%d_b" % (tag, rc), 0, b, rc=rc, seg="b", smp=smp_back(20))
    add(m, "back_first_b", 0, back_hit, seg="b", smp=smp_back(20))       # the pair in the other record order
    add(m, "back_first_f", 280, front_c, seg="f", smp=smp_front(20))
    add(m, "orphan_f", 280, front_hit, seg="f", smp=smp_front(20))
    add(m, "strands_f", 280, front_hit, rc=0, seg="f", smp=smp_front(20))
    add(m, "strands_b", 0, back_hit, rc=1, seg="b", smp=smp_back(20))
    add(m, "twice_f", 280, front_hit, seg="f", smp=smp_front(20))
    add(m, "twice_f", 280, front_c, seg="f", smp=smp_front(20))
    add(m, "twice_b", 0, back_hit, seg="b", smp=smp_back(20))
    add(m, "whole", 100, mutated(ref_at(m, 100, 50).replace("C", "A"), {}))
    n = len(m.rec)
    only_hit = np.ones(n, np.uint8)
    only_hit[0] = 0                                          # front0_f: the only hit of its molecule
    whole_molecule = np.ones(n, np.uint8)
    whole_molecule[[2, 3]] = 0                               # front1_f, front1_b
    whole_molecule[n - 4] = 0                                # an orphan
    return m, [only_hit, whole_molecule, np.zeros(n, np.uint8)]


def make_pile():
    m = mc._blank("pile_3000", 120, ms.Rng(9509), {})
    ref = list(m.ref_seq)
    ref[10], ref[59] = "C", "G"
    m.ref_seq = "".join(ref)
    seq = mutated(ref_at(m, 10, 50), {0: "T", 49: "A"})
    for k in range(3000):
        add(m, "p%d" % k, 10, seq)
    return m, []


def make_mixed(reverse):
    rng = ms.Rng(9510)
    L = 2000
    m = mc._blank("mixed", L, rng, {})
    for k in range(2000):
        n = int(rng.integers(20, 120, 1)[0])
        rc = int(rng.integers(0, 2, 1)[0])
        wrap = k % 33 == 0
        start = L - int(rng.integers(5, n - 5, 1)[0]) if wrap else int(rng.integers(0, L - n, 1)[0])
        cols = "".join(m.ref_seq[(start + i) % L] for i in range(n))
        read = revcomp(cols) if rc else cols
        read = deaminate(read, rng, 0.35 if k % 3 else 0.0, 0.01)
        u = rng.random(n)
        read = "".join("-" if u[i] < 0.02 else ("ACGT"[int(u[i] * 4000) % 4] if u[i] < 0.04 else ch) for i, ch in enumerate(read))
        stored = revcomp(read) if rc else read
        smp = mc._smp(n)
        if wrap:
            cut = L - start
            add(m, "m%d_f" % k, start, stored[:cut], rc=rc, seg="f", smp=smp[:cut], dr=k % 17 == 0)
            add(m, "m%d_b" % k, 0, stored[cut:], rc=rc, seg="b", smp=smp[cut:], dr=k % 17 == 0)
        else:
            add(m, "m%d" % k, start, stored, rc=rc, dr=k % 13 == 0)
    m.rec = [m.rec[i] for i in rng.permutation(len(m.rec)).tolist()]
    if reverse:
        m.rec = m.rec[::-1]
        m.ref_id = "mixed_reversed"
    dr = np.array([0 if r["dr"] else 1 for r in m.rec], np.uint8)
    return m, [dr]


def make_case(name):
    return {"hand": make_hand, "empty": make_empty, "lens": make_lens, "offsets": make_offsets, "edge_before": lambda: make_edge(False),
            "edge_behind": lambda: make_edge(True), "mirror": make_mirror, "odd": make_odd, "wrap": make_wrap, "pile_3000": make_pile,
            "mixed": lambda: make_mixed(False), "mixed_reversed": lambda: make_mixed(True)}[name]()


_cache = {}


def case(name):
    """(Maln, [use masks])"""
    if name not in _cache:
        _cache[name] = make_case(name)
    return _cache[name]


def uses(name):
    """None and the case's masks"""
    return [None] + case(name)[1]


# ---- the two read sets the compiled reference aligns for tests/golden/ma_damage (tools/make_ma_damage_goldens.py) -------------------
READ_SETS = ("reads_a", "reads_b")


def read_set(name, seed):
    """(reference FASTA, reads FASTA): a 600-base circular reference and 200 reads of 40 .. 90 bases with simulated damage, both strands,
    every eighth across the origin"""
    rng = ms.Rng(seed)
    L = 600
    ref = mc.ACGT[rng.integers(0, 4, L)].tobytes().decode()
    reads = []
    for k in range(200):
        n = int(rng.integers(40, 91, 1)[0])
        pos = L - int(rng.integers(12, n - 12, 1)[0]) if k % 8 == 1 else int(rng.integers(0, L - n, 1)[0])
        rc = int(rng.integers(0, 2, 1)[0])
        cols = "".join(ref[(pos + i) % L] for i in range(n))
        read = deaminate(revcomp(cols) if rc else cols, rng, (0.0, 0.9, 0.9, 0.5)[k % 4], 0.08 if k % 4 else 0.0)
        reads.append(">q%d\n%s\n" % (k, read))
    return ">%s\n%s\n" % (name, ref), "".join(reads)
