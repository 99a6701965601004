"""The .maln files of the duplicate consensus (ma_hip -u -j; MiaHip.ma_collapse): the smallest shapes at which the kernels of
csrc/mia_ma_collapse_kernels.h can go wrong.  Rebuilt from fixed seeds on maln_synth's Maln and the helpers of maln_dedup_cases;
nothing here is committed as text.  What matters here beside START, END, RC, SEG, SCORE and the IDs are the SEQ strings: a cluster is
one `truth` over the reference's columns and copies of it with substitutions, '-' and other characters.

  hand            a cluster of three whose representative loses a column, ties on one and keeps its lower case, a reverse cluster of two
                  (a tie that keeps `own`, one that gives N), a singleton.  Its results are written out by hand in the CPU test.
  empty, one, singletons    no record; one record; only clusters of one molecule: no launch, SEQ' is SEQ
  sizes           clusters of 2, 3, K - 1, K, K + 1 and 2 K + 1 members on both strands behind 5, 0 and 63 singletons, so that they begin
                  at several places of a chunk of K sorted entries: inside one chunk, across one boundary, across two
  columns         representatives of 1, 2, 15, 16, 17, 63, 64, 65, 255, 256 and 257 columns, clusters of three
  pile_5000, pile_70000 (library only)   one key: 79 and 1 094 work units add into one count array
  last_rep, last_member    the last record of the file is the representative / a member: its last column ends the SEQ buffer
  wrap            a representative that is an f / b pair with paired members; under t = 7 a whole member that votes on the front half
  jitter          members that start before and after the representative and end before and after it (t = 1, 2, 7)
  votes           '-' winning in the middle; a base over the representative's '-'; '-' votes at the first and last column; ties that
                  keep own and ties that give N; lower-case own; N and IUPAC voters
  dropped         a dropped member, a dropped representative, a cluster whose voters are all dropped
  inputs          NUM_INPUTS above 1 in members
  rep_given_last  the representative is the last record of the file and the best of its run
  mixed           20 000 records in clusters of 1 .. 40 with a jitter of 0 .. 2 columns, both strands, pairs over the origin; every copy
                  carries 0 .. 2 substitutions and now and then a '-'
  minority_ct     (end to end only) the kept copy alone reads T at position 1 where the reference has C: -u -D 3 keeps the cluster,
                  -u -j -D 3 does not
"""
import maln_ace_cases as mc
import maln_dedup_cases as dc
import maln_synth as ms

K = 64                                                      # members of a work unit of the count stage (MA_COL_K)
SIZES = (2, 3, K - 1, K, K + 1, 2 * K + 1)
COLUMNS = (1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257)
CASES = ("hand", "empty", "one", "singletons", "sizes", "columns", "pile_5000", "last_rep", "last_member", "wrap", "jitter", "votes", "dropped", "inputs",
         "rep_given_last", "mixed")
LIBRARY_ONLY = ("pile_70000",)
TOLERANCES = (0, 1, 2, 7)
OTHER = {"A": "C", "C": "G", "G": "T", "T": "A"}


def _put(m, rid, start, seq, rc=0, seg="n", score=0, dr=0, num_inputs=1):
    """a record whose columns start .. start + len(seq) - 1 read `seq`"""
    m.rec.append({"id": rid, "desc": "", "score": int(score), "num_inputs": num_inputs, "start": int(start), "end": int(start) + len(seq) - 1, "rc": int(rc), "tr": 0,
                  "dr": dr, "seg": seg, "seq": seq, "smp": mc._smp(len(seq)), "ins": []})


def _ref(m, start, n):
    return m.ref_seq[start:start + n]


def _mutate(rng, text, subs, dash=0.0):
    """`subs` substitutions and, with probability `dash`, one '-', none of them at the first or last column"""
    s = list(text)
    if len(s) > 2:
        for at in rng.integers(1, len(s) - 1, subs).tolist():
            s[at] = OTHER.get(s[at], "A")
        if dash and rng.random(1)[0] < dash:
            s[int(rng.integers(1, len(s) - 1, 1)[0])] = "-"
    return "".join(s)


def _cluster(m, rng, tag, start, n, size, rc=0, best=None):
    """`size` copies of the reference's columns start .. start + n - 1 with 0 .. 2 substitutions each; copy `best` has the best score"""
    scores = rng.integers(0, 500, size).tolist()
    subs = rng.integers(0, 3, size).tolist()
    best = size // 2 if best is None else best
    for k in range(size):
        _put(m, "%s_%d" % (tag, k), start, _mutate(rng, _ref(m, start, n), subs[k], 0.2), rc=rc, score=900 if k == best else scores[k])


def make_hand():
    m = mc._blank("hand", 60, ms.Rng(9701), {})
    m.ref_seq = "ACGTACGTAC" + "GATTACAGAT" + m.ref_seq[20:]
    #                       columns 2 .. 9:  G T A C G T A C
    _put(m, "a_rep", 2, "GTAcGTAC", score=50)               # the representative: the best score
    _put(m, "a_1", 2, "GTACGAAC", score=10)                 # column 5 (T>A) twice against the representative's T: becomes A
    _put(m, "a_2", 2, "GCACGAA-", score=20)                 # column 1: T T C stays; column 3: c C C, lower case stays; column 7: '-' at the edge does not count
    #                       columns 10 .. 15: G A T T A C
    _put(m, "b_0", 10, "GATTAC", rc=1, score=5)
    _put(m, "b_rep", 10, "GCTNAC", rc=1, score=9)           # column 1: C against A, a tie with own C: stays; column 3: own N, one T: becomes T
    _put(m, "c_0", 20, "ACAGA", rc=1, score=1)
    _put(m, "c_rep", 20, "ANRGA", rc=1, score=2, dr=1)      # dropped: does not vote.  column 1: one C, own N: C; column 2: one A over R: A
    _put(m, "d_0", 30, "TTTTT", score=1)                    # (the reference's own columns do not matter here)
    _put(m, "d_1", 30, "TGTTT", score=2)
    _put(m, "d_rep", 30, "TATTT", score=3)                  # column 1: T, G and A tie, own A is one of them: stays
    _put(m, "e_0", 40, "CCCCC", score=1)
    _put(m, "e_1", 40, "CGCCC", score=1)
    _put(m, "e_rep", 40, "CACCC", score=3, dr=1)            # dropped: C and G tie, own A is not among them: N
    _put(m, "single", 50, "ACGT", score=1)
    return m


def make_small(name):
    m = mc._blank(name, 400, ms.Rng(9702), {})
    if name == "one":
        _put(m, "only", 7, _ref(m, 7, 50), rc=1, score=-3)
    if name == "singletons":
        for k in range(70):
            _put(m, "s%d" % k, 3 * k, _mutate(ms.Rng(9703 + k), _ref(m, 3 * k, 40), 1), rc=k % 2, score=k)
    return m


def make_sizes():
    rng = ms.Rng(9710)
    m = mc._blank("sizes", 9000, rng, {})
    at = 0
    for rc in (1, 0):                                       # (reverse molecules come first in the sorted order)
        for lead in (5, 0, 63):
            for k in range(lead):
                _put(m, "s%d_%d" % (at, k), at, _ref(m, at, 30 + k), rc=rc, score=k)
            at += 1
            for size in SIZES:
                _cluster(m, rng, "g%d" % at, at, 40 + size % 7, size, rc=rc)
                at += 1
    return dc._shuffle(m, rng)


def make_columns():
    rng = ms.Rng(9720)
    m = mc._blank("columns", 4000, rng, {})
    for k, n in enumerate(COLUMNS):
        _cluster(m, rng, "n%d" % n, 300 * k, n, 3, rc=k % 2)
    return dc._shuffle(m, rng)


def make_pile(n):
    rng = ms.Rng(9730 + n % 89)
    m = mc._blank("pile_%d" % n, 200, rng, {})
    truth = _ref(m, 10, 70)
    subs = rng.integers(0, 3, n).tolist()
    score = rng.integers(-500, 500, n)
    score[n // 3] = 777
    for k in range(n):
        if k == n // 2:
            _put(m, "other", 10, _ref(m, 10, 71), score=900)
        # the representative disagrees with the pile on columns 5 and 6; column 40 is a '-' in two copies of three
        s = list(_mutate(rng, truth, subs[k]))
        if k == n // 3:
            s[5], s[6] = OTHER[truth[5]], "-"
        if k % 3:
            s[40] = "-"
        _put(m, "p%d" % k, 10, "".join(s), score=score[k])
    return m


def make_last(member):
    rng = ms.Rng(9740 + member)
    m = mc._blank("last_member" if member else "last_rep", 300, rng, {})
    _cluster(m, rng, "x", 5, 33, 4)
    truth = _ref(m, 200, 47)
    _put(m, "y_0", 200, _mutate(rng, truth, 1), score=500 if member else 3)
    _put(m, "y_1", 200, _mutate(rng, truth, 2), score=4)
    _put(m, "y_2", 200, truth[:-1] + OTHER[truth[-1]], score=5 if member else 500)           # the last record of the file, its last column differs
    return m


def make_wrap():
    rng = ms.Rng(9750)
    m = mc._blank("wrap", 300, rng, {})
    L = m.L
    for rc in (0, 1):
        t = "r" if rc else "f"
        front, back = _ref(m, 270, 30), _ref(m, 0, 20)
        for k, score in enumerate((40, 90, 41)):            # three pairs on one key: the second is the representative
            _put(m, "w%d%s_f" % (k, t), 270, _mutate(rng, front, 1 + k % 2), rc=rc, seg="f", score=score)
            _put(m, "w%d%s_b" % (k, t), 0, _mutate(rng, back, 1), rc=rc, seg="b", score=1)
        # within t = 7 of the pairs: a pair that ends four columns later, a whole record that ends on the reference's last column (it
        # votes on the front half alone), a pair that starts three columns later
        _put(m, "w3%s_f" % t, 270, _mutate(rng, front, 2), rc=rc, seg="f", score=20)
        _put(m, "w3%s_b" % t, 0, _mutate(rng, _ref(m, 0, 24), 2), rc=rc, seg="b", score=1)
        _put(m, "whole%s" % t, 270, front[:12] + OTHER[front[12]] + front[13:], rc=rc, score=10)
        _put(m, "w4%s_b" % t, 0, _mutate(rng, _ref(m, 0, 18), 1), rc=rc, seg="b", score=1)
        _put(m, "w4%s_f" % t, 273, _mutate(rng, _ref(m, 273, 27), 1), rc=rc, seg="f", score=15)
    _put(m, "orphan_f", 270, _ref(m, 270, 30), seg="f", score=40)
    return m


def make_jitter():
    rng = ms.Rng(9760)
    m = mc._blank("jitter", 2000, rng, {})
    for g, rc in enumerate((0, 1, 0, 1)):
        a, n = 100 + 400 * g, 60 + g
        truth = _ref(m, a - 10, n + 20)                     # columns a - 10 ..
        for k, (ds, de) in enumerate(((0, 0), (1, 0), (0, 1), (-1, -1), (2, -2), (-2, 2), (1, 1), (7, 0), (0, -7), (-5, 5), (0, 0))):
            text = truth[10 + ds:10 + n + de]
            _put(m, "j%d_%d" % (g, k), a + ds, _mutate(rng, text, k % 3), rc=rc, score=300 if k == 0 and g < 2 else 50 + k)
    return dc._shuffle(m, rng)


def make_votes():
    m = mc._blank("votes", 400, ms.Rng(9770), {})
    t = _ref(m, 10, 12)

    def with_(text, **at):
        s = list(text)
        for k, ch in at.items():
            s[int(k[1:])] = ch
        return "".join(s)

    # '-' wins in the middle (column 4); a base replaces the representative's '-' (column 6); '-' at the first and last column of two of
    # three copies: not counted, the base stays
    _put(m, "g_rep", 10, with_(t, c6="-"), score=9)
    _put(m, "g_1", 10, with_(t, c4="-", c0="-", c11="-"), score=1)
    _put(m, "g_2", 10, with_(t, c4="-", c0="-", c11="-"), score=2)
    # ties: two against two with own among them (column 3), A and G against own C (column 5: N), lower-case own that wins (column 7),
    # lower-case own that loses (column 8), N and IUPAC voters that are no vote (columns 9, 10)
    u = _ref(m, 100, 12)
    x, y = OTHER[u[5]], OTHER[OTHER[u[5]]]
    _put(m, "t_rep", 100, with_(u, c7=u[7].lower(), c8=u[8].lower()), score=9, rc=1)
    _put(m, "t_1", 100, with_(u, c3=OTHER[u[3]], c5=x, c8=OTHER[u[8]], c9="N", c10="R"), score=1, rc=1)
    _put(m, "t_2", 100, with_(u, c3=OTHER[u[3]], c5=y, c8=OTHER[u[8]], c9="N", c10="Y"), score=2, rc=1)
    _put(m, "t_3", 100, with_(u, c5=x, c7=u[7].lower(), c8=OTHER[u[8]], c9="n", c10="K"), score=3, rc=1)
    _put(m, "t_5", 100, with_(u, c3="N", c5=y), score=4, rc=1)                                  # column 5: x and y two each, own once: N
    _put(m, "t_4", 100, with_(u, c5=y, c10=OTHER[u[10]].lower()), score=3, rc=1, dr=1)          # dropped: with vote = not DR it is out of every column
    # the representative's own edge '-' (a hand-made file): a single winner replaces it, '-' votes there still do not count
    w = _ref(m, 200, 8)
    _put(m, "e_rep", 200, "-" + w[1:], score=9)
    _put(m, "e_1", 200, "-" + w[1:], score=1)
    _put(m, "e_2", 200, w, score=2)
    return m


def make_dropped():
    rng = ms.Rng(9780)
    m = mc._blank("dropped", 900, rng, {})
    for g, dropped in enumerate(((1,), (0,), (0, 1, 2), (2, 3))):           # copy 0 is the representative
        truth = _ref(m, 50 + 200 * g, 55)
        for k in range(4 if g < 3 else 5):
            text = truth if k == 0 else _mutate(rng, truth[:20] + OTHER[truth[20]] + truth[21:], 1)
            _put(m, "d%d_%d" % (g, k), 50 + 200 * g, text, rc=g % 2, score=100 - k, dr=1 if k in dropped or (g == 2 and k == 3) else 0)
    return m


def make_inputs():
    rng = ms.Rng(9790)
    m = mc._blank("inputs", 600, rng, {})
    for g, inputs in enumerate(((1, 3, 5), (2, 2), (7, 1, 1, 40000), (None, 2))):            # None: the record has no NUM_INPUTS line
        for k, ni in enumerate(inputs):
            _put(m, "i%d_%d" % (g, k), 20 + 100 * g, _mutate(rng, _ref(m, 20 + 100 * g, 44), 1), score=k, num_inputs=ni, dr=1 if (g, k) == (2, 1) else 0)
    _put(m, "i_pair_f", 570, _ref(m, 570, 30), seg="f", score=9, num_inputs=4)
    _put(m, "i_pair_b", 0, _ref(m, 0, 10), seg="b", score=9, num_inputs=4)
    _put(m, "i_pair2_f", 570, _ref(m, 570, 30), seg="f", score=8, num_inputs=6)
    _put(m, "i_pair2_b", 0, _ref(m, 0, 10), seg="b", score=8, num_inputs=9)              # a back half's NUM_INPUTS does not count
    return m


def make_rep_given_last():
    rng = ms.Rng(9800)
    m = mc._blank("rep_given_last", 300, rng, {})
    _put(m, "alone", 5, _ref(m, 5, 40), score=1)
    truth = _ref(m, 100, 66)
    for k in range(6):
        _put(m, "r%d" % k, 100, _mutate(rng, truth[:30] + OTHER[truth[30]] + truth[31:], 1), rc=1, score=10 + k)
    _put(m, "r_rep", 100, truth, rc=1, score=99)
    return m


def make_mixed():
    """maln_dedup_cases.make_mixed_20000's shape; a cluster's copies are one truth with 0 .. 2 substitutions and an occasional '-'"""
    rng = ms.Rng(9810)
    L = 16000
    m = mc._blank("mixed", L, rng, {})
    pairs = 0
    while len(m.rec) < 20000:
        size = min(int(rng.integers(1, 41, 1)[0]), 20000 - len(m.rec))
        rc = int(rng.integers(0, 2, 1)[0])
        n = int(rng.integers(30, 121, 1)[0])
        wrap = pairs < 200 and len(m.rec) % 3 == 0 and size >= 2
        a = L - int(rng.integers(5, n - 5, 1)[0]) if wrap else int(rng.integers(0, L - n - 4, 1)[0])
        jit = rng.integers(0, 3, 2 * size)
        score = rng.integers(-300, 3000, size)
        subs = rng.integers(0, 3, size).tolist()
        for k in range(size):
            if len(m.rec) + (2 if wrap else 1) > 20000:
                break
            s, e = a + int(jit[2 * k]), a + n - 1 + int(jit[2 * k + 1])
            rid = "c%d_%d" % (len(m.rec), k)
            if wrap and pairs < 200:
                _put(m, rid + "_f", s, _mutate(rng, _ref(m, s, L - s), subs[k], 0.1), rc=rc, seg="f", score=score[k])
                _put(m, rid + "_b", 0, _mutate(rng, _ref(m, 0, e - L + 1), 1), rc=rc, seg="b", score=score[k] - 1)
                pairs += 1
            elif wrap:
                break
            else:
                _put(m, rid, s, _mutate(rng, _ref(m, s, e - s + 1), subs[k], 0.1), rc=rc, score=score[k], dr=1 if k % 17 == 16 else 0)
    return dc._shuffle(m, rng)


def make_minority_ct():
    """three copies; the kept one alone reads T over the reference's C at its first position"""
    m = mc._blank("minority_ct", 200, ms.Rng(9820), {})
    m.ref_seq = m.ref_seq[:40] + "C" + m.ref_seq[41:]
    truth = _ref(m, 40, 50)                                 # (every other column reads as the reference: no other hit)
    _put(m, "kept", 40, "T" + truth[1:], score=90)
    _put(m, "copy1", 40, truth, score=10)
    _put(m, "copy2", 40, truth, score=20)
    return m


def make_case(name):
    if name.startswith("pile_"):
        return make_pile(int(name[5:]))
    if name in ("empty", "one", "singletons"):
        return make_small(name)
    return {"hand": make_hand, "sizes": make_sizes, "columns": make_columns, "last_rep": lambda: make_last(0), "last_member": lambda: make_last(1),
            "wrap": make_wrap, "jitter": make_jitter, "votes": make_votes, "dropped": make_dropped, "inputs": make_inputs,
            "rep_given_last": make_rep_given_last, "mixed": make_mixed, "minority_ct": make_minority_ct}[name]()


_cache = {}


def case(name):
    if name not in _cache:
        _cache[name] = make_case(name)
    return _cache[name]
