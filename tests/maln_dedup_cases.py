"""The .maln files of the duplicate filter (ma_hip -u, -t; MiaHip.ma_dedup): the smallest shapes at which the kernels of
csrc/mia_ma_dedup_kernels.h can go wrong.  Rebuilt from fixed seeds on maln_synth's Maln and writer; nothing here is committed as text.
A record's columns are the reference's own characters: what matters here are START, END, RC, SEG, SCORE, the IDs and the inserts.

  hand              the two quirks of the walk ("Duplicate filter": the latest anchor only), a run whose best molecule is
                    the last in the file, a score tie and negative scores.  Its results are written out by hand in the CPU test.
  empty, one        no record (no launch), one record (one run)
  pile_63 .. 257    one run of that many molecules and one other molecule: a run across lanes, wavefronts and workgroups
  pile_5000, pile_70000 (library only: counts beyond 16 bits, one atomic per workgroup and not per molecule)
  runs_edge         forward runs of 255, 256 and 257 molecules that begin one entry before, on and one entry behind a multiple of 256
                    in the sorted order (a workgroup of the run stage takes 256 entries)
  stairs_4097       forward runs a = 0 .. 4096, e = a + 50: with t = 1 the anchors are the even a, with t = 2 every third -- a restart
                    per workgroup or per doubling round changes the parity; 13 doubling rounds
  stairs_rev        the same on the reverse strand, where the walk goes e downwards
  e_ladder          forward: one a, e = 300 .. 200; reverse: one e, a = 10 .. 110: the window in the second coordinate
  strand_seam       the last reverse run and the first forward run have the same coordinates: never one cluster
  wrap              pairs over the origin against whole molecules with the same start; orphans: no mate, a stem twice, strands differ,
                    an ID without the suffix
  ins_only_in_dups  inserts that only molecules which are not kept carry: GAPS falls there, stays where a kept record has one, and
                    falls to the kept record's length where both have one
  ins_repeat        (not in CASES: for the GAPS line alone) a kept record with two pairs for one position: the later one counts
  mixed_20000       20 000 records in clusters of 1 .. 40 with a jitter of 0 .. 2 columns, both strands, 200 pairs over the origin
"""
import maln_ace_cases as mc
import maln_synth as ms

PILES = (63, 64, 65, 255, 256, 257, 5000)
CASES = ("hand", "empty", "one") + tuple("pile_%d" % n for n in PILES) + ("runs_edge", "stairs_4097", "stairs_rev", "e_ladder", "strand_seam",
                                                                         "wrap", "ins_only_in_dups", "mixed_20000")
LIBRARY_ONLY = ("pile_70000",)
TOLERANCES = (0, 1, 2, 7, 100)
WG = 256                                                    # entries of a workgroup of the run stage (MAD_THREADS)


def _add(m, rid, start, end, rc=0, seg="n", score=0, ins=(), dr=0):
    """columns start .. end (end = start - 1: none) of the reference"""
    n = end - start + 1
    seq = "".join(m.ref_seq[(start + k) % m.L] for k in range(n))
    m.rec.append({"id": rid, "desc": "", "score": int(score), "num_inputs": 1, "start": int(start), "end": int(end), "rc": int(rc), "tr": 0, "dr": dr,
                  "seg": seg, "seq": seq, "smp": mc._smp(n), "ins": list(ins)})
    for pos, text in ins:
        if 0 < pos < n and start + pos < m.L:
            m.gaps[start + pos] = max(int(m.gaps[start + pos]), len(text))


def _shuffle(m, rng):
    m.rec = [m.rec[i] for i in rng.permutation(len(m.rec)).tolist()]
    return m


def make_hand():
    m = mc._blank("hand", 400, ms.Rng(9401), {})
    for rid, rc, s, e, score in (("h0", 0, 0, 100, 10), ("h1", 0, 0, 90, 10), ("h2", 0, 1, 100, 10), ("r_low", 1, 50, 120, -9), ("r_a", 1, 50, 120, -5),
                                 ("r_b", 1, 50, 120, -5), ("q0", 0, 200, 300, 7), ("q1", 0, 201, 300, 8), ("q2", 0, 202, 300, 9), ("q3", 0, 203, 300, 6),
                                 ("h0_again", 0, 0, 100, 11)):
        _add(m, rid, s, e, rc=rc, score=score)
    return m


def make_small(name):
    m = mc._blank(name, 120, ms.Rng(9402), {})
    if name == "one":
        _add(m, "only", 7, 60, rc=1, score=-3)
    return m


def make_pile(n):
    rng = ms.Rng(9410 + n % 97)
    m = mc._blank("pile_%d" % n, 120, rng, {})
    score = rng.integers(-500, 500, n)
    score[[n // 3, n - 2]] = 777                            # the best twice: the lower index wins
    other = n // 2
    for k in range(n):
        if k == other:
            _add(m, "other", 10, 61, score=900)
        _add(m, "p%d" % k, 10, 60, rc=0, score=score[k])
    return m


def make_runs_edge():
    rng = ms.Rng(9420)
    m = mc._blank("runs_edge", 6000, rng, {})
    at, a = 0, 0                                            # entries so far in the sorted order, next free start
    for size in (255, 256, 257):
        for off in (WG - 1, 0, 1):
            while at % WG != off:                           # single molecules up to the place the run has to begin at
                _add(m, "s%d" % a, a, a + 40, score=int(rng.integers(-50, 50, 1)[0]))
                a, at = a + 1, at + 1
            score = rng.integers(-9, 9, size)               # many ties
            for k in range(size):
                _add(m, "g%d_%d" % (a, k), a, a + 40, score=score[k])
            a, at = a + 1, at + size
    return _shuffle(m, rng)


def make_stairs(rev):
    rng = ms.Rng(9430 + rev)
    m = mc._blank("stairs_rev" if rev else "stairs_4097", 4200, rng, {})
    for k in range(4097):
        if rev:
            _add(m, "v%d" % k, 4100 - k, 4150 - k, rc=1, score=k % 5)
        else:
            _add(m, "u%d" % k, k, k + 50, score=k % 5)
    return _shuffle(m, rng)


def make_e_ladder():
    rng = ms.Rng(9440)
    m = mc._blank("e_ladder", 400, rng, {})
    for e in range(200, 301):
        _add(m, "f%d" % e, 10, e, score=e % 7)
    for a in range(10, 111):
        _add(m, "r%d" % a, a, 300, rc=1, score=a % 3)
    return _shuffle(m, rng)


def make_strand_seam():
    m = mc._blank("strand_seam", 200, ms.Rng(9450), {})
    _add(m, "rev_first", 20, 90, rc=1, score=5)
    _add(m, "rev_last", 5, 40, rc=1, score=5)
    _add(m, "fwd_first", 5, 40, rc=0, score=6)
    _add(m, "fwd_next", 30, 80, rc=0, score=5)
    return m


def make_wrap():
    m = mc._blank("wrap", 300, ms.Rng(9460), {})
    L = m.L
    for rc in (0, 1):
        t = "r" if rc else "f"
        _add(m, "w1%s_f" % t, 280, L - 1, rc=rc, seg="f", score=40)         # a = 280, e = 19 + L
        _add(m, "whole%s" % t, 280, L - 1, rc=rc, score=90)                 # the same start, not the same molecule
        _add(m, "w1%s_b" % t, 0, 19, rc=rc, seg="b", score=1)
        _add(m, "w2%s_b" % t, 0, 19, rc=rc, seg="b", score=2)               # the same molecule again, better: back half first in the file
        _add(m, "w2%s_f" % t, 280, L - 1, rc=rc, seg="f", score=41)
        _add(m, "w3%s_f" % t, 280, L - 1, rc=rc, seg="f", score=99)         # another back end: a molecule of its own (within t = 7)
        _add(m, "w3%s_b" % t, 0, 25, rc=rc, seg="b", score=99)
        _add(m, "back_alone%s" % t, 0, 19, rc=rc, score=3)                  # whole, the back half's columns
    _add(m, "no_mate_f", 280, L - 1, seg="f", score=40)                     # orphans ...
    _add(m, "twice_f", 281, L - 1, seg="f", score=40)
    _add(m, "twice_f", 281, L - 1, seg="f", score=41)
    _add(m, "twice_b", 0, 19, seg="b", score=40)
    _add(m, "strands_f", 282, L - 1, rc=0, seg="f", score=40)
    _add(m, "strands_b", 0, 19, rc=1, seg="b", score=40)
    _add(m, "no_suffix", 280, L - 1, seg="f", score=40)
    return m


def make_ins_only_in_dups():
    m = mc._blank("ins_only_in_dups", 200, ms.Rng(9470), {})
    _add(m, "dup1", 20, 70, score=50, ins=[(10, "A"), (10, "AC"), (20, "ACG")])      # GAPS[30] = 2, GAPS[40] = 3
    _add(m, "best", 20, 70, score=80, ins=[(20, "A")])                      # kept: GAPS[30] -> 0, GAPS[40] -> 1
    _add(m, "dup2", 20, 70, score=60, ins=[(10, "T"), (30, "GG")])          # GAPS[50] = 2 -> 0
    _add(m, "alone", 100, 150, score=10, ins=[(5, "TT")])                   # kept: GAPS[105] = 2 stays
    _add(m, "alone_rev", 100, 150, rc=1, score=10, ins=[(7, "C")])          # GAPS[107] = 1 stays
    return m


def make_ins_repeat():
    """a kept record that gives two pairs for one position: the later one counts, as in read_ma.  Only for the GAPS line of the
    filtered file (-m): the tally of a file with such pairs is not this filter's business"""
    m = mc._blank("ins_repeat", 200, ms.Rng(9471), {})
    _add(m, "kept", 20, 70, score=80, ins=[(5, "GGG"), (5, "T"), (9, "A"), (9, "CC")])     # GAPS[25] = 3 -> 1, GAPS[29] = 2 stays
    _add(m, "gone", 20, 70, score=10, ins=[(5, "AC"), (30, "ACGT")])                       # GAPS[50] = 4 -> 0
    return m


def make_mixed_20000():
    rng = ms.Rng(9480)
    L = 16000
    m = mc._blank("mixed_20000", L, rng, {})
    pairs = 0
    while len(m.rec) < 20000:
        size = min(int(rng.integers(1, 41, 1)[0]), 20000 - len(m.rec))
        rc = int(rng.integers(0, 2, 1)[0])
        n = int(rng.integers(30, 121, 1)[0])
        wrap = pairs < 200 and len(m.rec) % 3 == 0 and size >= 2
        a = L - int(rng.integers(5, n - 5, 1)[0]) if wrap else int(rng.integers(0, L - n - 4, 1)[0])
        jit = rng.integers(0, 3, 2 * size)
        score = rng.integers(-300, 3000, size)
        for k in range(size):
            if len(m.rec) + (2 if wrap else 1) > 20000:
                break
            s, e = a + int(jit[2 * k]), a + n - 1 + int(jit[2 * k + 1])
            rid = "c%d_%d" % (len(m.rec), k)
            if wrap and pairs < 200:
                _add(m, rid + "_f", s, L - 1, rc=rc, seg="f", score=score[k])
                _add(m, rid + "_b", 0, e - L, rc=rc, seg="b", score=score[k] - 1)
                pairs += 1
            elif wrap:
                break
            else:
                _add(m, rid, s, e, rc=rc, score=score[k])
    return _shuffle(m, rng)


def make_pile_70000():
    return make_pile(70000)


def make_case(name):
    if name.startswith("pile_"):
        return make_pile(int(name[5:]))
    if name in ("empty", "one"):
        return make_small(name)
    return {"hand": make_hand, "runs_edge": make_runs_edge, "stairs_4097": lambda: make_stairs(0), "stairs_rev": lambda: make_stairs(1),
            "e_ladder": make_e_ladder, "strand_seam": make_strand_seam, "wrap": make_wrap, "ins_only_in_dups": make_ins_only_in_dups,
            "ins_repeat": make_ins_repeat, "mixed_20000": make_mixed_20000}[name]()


# ---- the two read sets the compiled reference aligns for tests/golden/ma_dedup (tools/make_ma_dedup_goldens.py) ----------------------
READ_SETS = ("reads_a", "reads_b")
_COMP = str.maketrans("ACGT", "TGCA")


def read_set(name):
    """(reference FASTA, reads FASTA): a 600-base circular reference and 160 reads drawn from 34 sites, four of them across the
    origin, both strands, 0 .. 2 substitutions each and, in the second set, inserts of 1 .. 3 bases"""
    second = name == "reads_b"
    rng = ms.Rng(9490 + int(second))
    L = 600
    ref = mc.ACGT[rng.integers(0, 4, L)].tobytes().decode()
    sites = []
    for k in range(34):
        n = int(rng.integers(45, 90, 1)[0])
        pos = L - int(rng.integers(10, n - 10, 1)[0]) if k < 4 else int(rng.integers(0, L - n, 1)[0])
        sites.append((pos, n, int(rng.integers(0, 2, 1)[0])))
    reads = []
    for k in range(160):
        pick = int(rng.integers(0, len(sites), 1)[0])
        pos, n, rc = sites[k % 4 if k < 24 else pick]       # (enough reads across the origin in either set)
        seq = [ref[(pos + i) % L] for i in range(n)]
        for _ in range(int(rng.integers(0, 3, 1)[0])):
            at = int(rng.integers(8, n - 8, 1)[0])
            seq[at] = "ACGT"[("ACGT".index(seq[at]) + 1 + int(rng.integers(0, 3, 1)[0])) % 4]
        if second and k % 3 == 0:
            at = int(rng.integers(12, n - 12, 1)[0])
            seq[at:at] = list(mc._bases(rng, int(rng.integers(1, 4, 1)[0])))
        text = "".join(seq)
        reads.append(">q%d\n%s\n" % (k, text.translate(_COMP)[::-1] if rc else text))
    return ">%s\n%s\n" % (name, ref), "".join(reads)


_cache = {}


def case(name):
    if name not in _cache:
        _cache[name] = make_case(name)
    return _cache[name]
