"""The three Myers kernels (csrc/mia_myers_kernels.h: k_myers_lanes, k_myers_ond, k_myers) and their router (myers_run) against
the plain dynamic programme of tests/myers_ref.py, on every route -- default, MIA_HIP_MYERS_NO_LANES, MIA_HIP_MYERS_NO_OND, both --
at the kernels' block, lane and cap edges.  Every comparison is elementwise equality with the programme; every test also asserts,
on the programme's answers alone, that its cases are not vacuous.  The cases come from seeds (no golden file); the functions that
make them import no GPU code, so their reference answers can be looked at without one."""
import functools
import os

import numpy as np
import pytest

import myers_ref
from myers_ref import NONE

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", np.uint8)
IUPAC = np.frombuffer(b"ACGTACGTACGTNRYKMSWBDHVacgtnX-", np.uint8)       # the alphabet of test_gpu_myers.py


class Cases:
    """pairs of one test: sequences as bytes, mode, maxd, and a tag per pair"""

    def __init__(self):
        self.A, self.B, self.mode, self.maxd, self.tag = [], [], [], [], []

    def add(self, a, b, mode, maxd, tag=""):
        self.A.append(bytes(a)); self.B.append(bytes(b)); self.mode.append(int(mode)); self.maxd.append(int(maxd)); self.tag.append(tag)
        return len(self.A) - 1

    def __len__(self):
        return len(self.A)

    @functools.cached_property
    def dist(self):
        """the programme's distances before maxd (computed once, shared by the tests that need them)"""
        d = myers_ref.myers_distance(self.A, self.B, self.mode)
        d.setflags(write=False)
        return d

    @functools.cached_property
    def want(self):
        total = np.array([len(a) + len(b) for a, b in zip(self.A, self.B)], np.int64)
        w = np.where(self.dist < np.minimum(np.array(self.maxd, np.int64), total), self.dist, NONE).astype(np.uint32)
        w.setflags(write=False)
        return w

    def take(self, idx):
        c = Cases()
        for i in idx:
            c.add(self.A[i], self.B[i], self.mode[i], self.maxd[i], self.tag[i])
        return c


def _rand(rng, alpha, n):
    return alpha[rng.integers(0, len(alpha), n)].copy()


def _edit(rng, a, alpha, n):
    """n single-character edits: substitutions, deletions, insertions"""
    b = list(a)
    for _ in range(n):
        if not b:
            break
        p = int(rng.integers(0, len(b)))
        u = rng.random()
        if u < 0.4:
            b[p] = alpha[rng.integers(0, len(alpha))]
        elif u < 0.7:
            del b[p]
        else:
            b.insert(p, alpha[rng.integers(0, len(alpha))])
    return np.array(b, np.uint8)


def _high(rng, s, k):
    """k characters of s overwritten with bytes 0x80..0xFF (no bitmap knows them)"""
    if len(s):
        s[rng.integers(0, len(s), k)] = rng.integers(0x80, 0x100, k)
    return s


# ---- (a) one pair per lane ------------------------------------------------------------------------------------------------------
LANE_LA = [0, 1, 2, 7, 8, 9, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 319, 320]
LANE_LB = [0, 1, 7, 8, 9, 63, 64, 65, 340]
LANE_GROUP = 640          # pairs 640 .. 703 are one wavefront of k_myers_lanes in the default context (64 pairs a wavefront, in order)


@functools.lru_cache(None)
def lane_cases():
    rng = np.random.default_rng(4101)
    c = Cases()
    for i in range(3008):
        alpha = ACGT if i % 4 < 2 else IUPAC
        la = int(rng.choice(LANE_LA)) if i % 3 == 0 else int(rng.integers(0, 321))
        a = _rand(rng, alpha, la)
        kind = i % 5
        if kind == 0:
            b = _rand(rng, alpha, int(rng.choice(LANE_LB)) if i % 2 == 0 else int(rng.integers(0, 341)))        # unrelated
        else:
            b = _edit(rng, a, alpha, int(rng.integers(0, 1 + la // (3 if kind == 1 else 12))))
            if kind == 2 and len(b) > 20:
                b = b[int(rng.integers(0, 10)):len(b) - int(rng.integers(0, 10))]                                 # overhangs (modes 1 and 2)
            if kind == 3 and i % 2:
                b = np.concatenate([b, _rand(rng, alpha, int(rng.integers(1, 30)))])[:340]
            b = b[:340]
        if i % 97 == 0:
            a, b = _high(rng, a, 3), _high(rng, b, 3)
        c.add(a, b, rng.integers(0, 3), rng.choice([1, 2, 5, 30, 100, 700, 100000]), "lane")
    # one wavefront with the extremes side by side: the loop over seq_b runs to the longest seq_b of the 64 lanes
    g = LANE_GROUP
    for k in range(64):
        alpha = ACGT if k % 2 else IUPAC
        if k % 8 == 0:
            a, b, m = _rand(rng, alpha, 320), b"", k // 8 % 3                       # lb = 0 beside lb = 340
        elif k % 8 == 1:
            a, b, m = _rand(rng, alpha, int(rng.integers(1, 321))), _rand(rng, alpha, 340), k // 8 % 3
        elif k % 8 == 2:
            a, b, m = b"", _rand(rng, alpha, int(rng.choice([0, 1, 340]))), k // 8 % 3          # la = 0 beside la = 320
        elif k % 8 == 3:
            a = _rand(rng, alpha, 320)
            b, m = _edit(rng, a, alpha, 6)[:340], k // 8 % 3
        elif k % 8 == 4:
            b = _rand(rng, alpha, 340)
            a, m = (b[200:205].copy() if k % 16 == 4 else _rand(rng, alpha, 5)), 1              # la = 5, lb = 340, all of seq_b
        elif k % 8 == 5:
            a = _rand(rng, alpha, 320)
            b, m = (a[:3].copy() if k % 16 == 5 else _rand(rng, alpha, 3)), 2                   # la = 320, lb = 3, all of seq_a
        else:
            continue                                                                            # (the random pair stays)
        c.A[g + k], c.B[g + k], c.mode[g + k], c.maxd[g + k] = bytes(a), bytes(b), m, 100000
    return c


# ---- (c) k_myers between 7 and 64 blocks, one block a lane ------------------------------------------------------------------------
@functools.lru_cache(None)
def block_cases():
    rng = np.random.default_rng(4103)
    c = Cases()
    n = 0
    for la in (321, 384, 385, 448, 449, 1024, 1025, 4032, 4033, 4095, 4096):
        for kind in ("unrelated", "tenth", "near"):
            for rep in range(2):
                alpha = ACGT if (n + rep) % 2 else IUPAC
                a = _rand(rng, alpha, la)
                lb = int(rng.integers(300, 1201))
                if kind == "unrelated":
                    b = _rand(rng, alpha, lb)
                else:
                    src = a[:min(la, lb)]
                    b = _edit(rng, src, alpha, len(src) // 10 if kind == "tenth" else int(rng.integers(0, 12)))[:1200]
                if n % 13 == 0:
                    a, b = _high(rng, a, 4), _high(rng, b, 4)
                c.add(a, b, n % 3, 100000, kind)
                n += 1
    return c


# ---- (d) k_myers with K >= 2 blocks a lane -----------------------------------------------------------------------------------------
K_LA = (4097, 4160, 8192, 8193, 12288, 12289, 16384, 16385, 32767, 32768)


@functools.lru_cache(None)
def k_short_b_cases():
    """every la, all three modes, seq_b of 100..600 characters: unrelated, and an edited prefix of seq_a"""
    rng = np.random.default_rng(4104)
    c = Cases()
    for n, la in enumerate(K_LA):
        alpha = ACGT if n % 2 else IUPAC
        a = _rand(rng, alpha, la)
        if n % 3 == 0:
            a = _high(rng, a, 5)
        for mode in (0, 1, 2):
            c.add(a, _rand(rng, alpha, int(rng.integers(100, 601))), mode, 100000, "unrelated")
            c.add(a, _edit(rng, a[:int(rng.integers(100, 590))], alpha, int(rng.integers(0, 10))), mode, 100000, "prefix")
    return c


@functools.lru_cache(None)
def k_long_b_cases():
    """seq_b about as long as seq_a: the carries through every block of every lane, the last lane, the scan of mode 1"""
    rng = np.random.default_rng(4105)
    c = Cases()
    for la in (4097, 8193):
        c.add(_rand(rng, ACGT, la), _rand(rng, ACGT, la - int(rng.integers(0, 50))), la % 3, 100000, "unrelated")
    for la in (4097, 8193, 16385):
        a = _rand(rng, IUPAC if la == 8193 else ACGT, la)
        b = _high(rng, _edit(rng, a, ACGT, 30), 2)
        for mode in (0, 1, 2):
            c.add(a, b, mode, 100000, "near")
    for la in (4097, 8193):                     # all of seq_b against a prefix of seq_a that ends in a high lane
        a = _rand(rng, ACGT, la)
        c.add(a, _edit(rng, a[:la - 100], ACGT, 25), 1, 100000, "high lane")
    for la in (4097, 8193, 16385):              # ... in a middle block of a middle lane
        a = _rand(rng, ACGT, la)
        c.add(a, _edit(rng, a[:la // 2 + 37], IUPAC, 25), 1, 100000, "middle lane")
    return c


# ---- (e) the D-path kernel's cap, straddled --------------------------------------------------------------------------------------
CAP_RANGES = ((330, range(140, 181)), (1000, range(235, 291)))
CAP_ALIGN = {330: range(156, 161), 1000: range(258, 264)}


@functools.lru_cache(None)
def cap_cases():
    """seq_b = seq_a with s distinct positions overwritten by X (X meets nothing: every one of them costs 1), s across the row
    counts at which k_myers_ond gives a pair of this size up; the prefix modes with 40 characters more on the side that need not
    be consumed"""
    rng = np.random.default_rng(4106)
    c = Cases()
    for la, srange in CAP_RANGES:
        for s in srange:
            for mode in (0, 1, 2):
                a = _rand(rng, ACGT, la)
                b = a.copy()
                b[rng.choice(la, s, replace=False)] = ord("X")
                if mode == 1:
                    a = np.concatenate([a, _rand(rng, ACGT, 40)])
                if mode == 2:
                    b = np.concatenate([b, _rand(rng, ACGT, 40)])
                if s % 17 == 0:
                    b[b == ord("X")] = rng.integers(0x80, 0x100, int((b == ord("X")).sum()))       # bytes no bitmap knows, for X
                for maxd in (100000, s, s + 1):
                    c.add(a, b, mode, maxd, "%d/%d" % (la, s))
    return c


# ---- (f) a second pair for a workgroup -------------------------------------------------------------------------------------------
GRID = 8192               # workgroups of k_myers_ond and of k_myers for a call of more long pairs than that: pair p + 8192 follows pair p


@functools.lru_cache(None)
def second_pair_cases():
    rng = np.random.default_rng(4107)
    n = 8500

    def handed_on(la):          # mode 0, a short unrelated seq_b: D >= la - lb > 260, no D-path cap of a pair this size reaches it
        return _rand(rng, ACGT, la), _rand(rng, ACGT, int(rng.integers(1, 61))), 0, 100000

    def finished(la):           # all of seq_b against a prefix of seq_a, a few edits: the D-path kernel answers
        a = _rand(rng, ACGT, la)
        return a, _edit(rng, a[:int(rng.integers(20, 58))], ACGT, int(rng.integers(0, 4))), 1, 100000

    def any_pair(la):
        alpha = ACGT if rng.random() < 0.5 else IUPAC
        a = _rand(rng, alpha, la)
        b = _rand(rng, alpha, int(rng.integers(0, 61))) if rng.random() < 0.5 else _edit(rng, a[:int(rng.integers(0, 58))], alpha, int(rng.integers(0, 4)))
        return a, b, int(rng.integers(0, 3)), int(rng.choice([3, 30, 100000]))

    slots = [None] * n
    for p in range(n - GRID):
        q = p + GRID
        seven, six = int(rng.integers(385, 401)), int(rng.integers(321, 385))      # 7 blocks, 6 blocks
        k = p % 6
        if k == 0:
            slots[p], slots[q] = handed_on(seven), finished(six)
        elif k == 1:
            slots[p], slots[q] = finished(seven), handed_on(six)
        elif k == 2:
            a, b, m, _ = any_pair(seven)
            slots[p], slots[q] = (a, b, m, int(rng.choice([0, -1]))), finished(six)                  # no distance admissible, then a pair
        elif k == 3:
            a, b, m, _ = any_pair(six)
            slots[p], slots[q] = handed_on(seven), (a, b, m, int(rng.choice([0, -5])))
        elif k == 4:
            slots[p], slots[q] = (_rand(rng, ACGT, seven), b"", int(rng.integers(0, 3)), 100000), any_pair(six)   # an empty seq_b, then a pair
        else:
            slots[p], slots[q] = any_pair(seven), (_rand(rng, IUPAC, six), b"", int(rng.integers(0, 3)), 100000)
    for p in range(n):
        if slots[p] is None:
            slots[p] = any_pair(int(rng.integers(321, 401)))
    c = Cases()
    for p, (a, b, m, maxd) in enumerate(slots):
        if p % 500 == 7:
            a = _high(rng, np.array(a), 2)
        c.add(a, b, m, maxd, "second" if p >= GRID else "")
    return c


# ---- (g) beyond the D-path kernel's LDS budget, (h) the other side far shorter ---------------------------------------------------
@functools.lru_cache(None)
def lds_cases():
    """321 x 310 000: the two packed sequences alone are more than the 150 KB k_myers_ond may use, so the pair has no cap and k_myers
    answers it alone.  Beside it a pair the D-path kernel takes and one for a lane."""
    rng = np.random.default_rng(4108)
    c = Cases()
    a, b = _rand(rng, ACGT, 321), _high(rng, _rand(rng, ACGT, 310_000), 50)
    c.add(a, b, 2, 400_000, "huge")              # (alone in its call)
    c.add(a, b, 0, 400_000, "huge")
    c.add(a, b, 2, 400_000, "huge")
    x = _rand(rng, IUPAC, 900)
    c.add(x, _edit(rng, x, ACGT, 12), 0, 100000, "dpath")
    y = _rand(rng, ACGT, 200)
    c.add(y, _edit(rng, y, ACGT, 9), 0, 100000, "lane")
    return c


@functools.lru_cache(None)
def short_side_cases():
    rng = np.random.default_rng(4109)
    c = Cases()
    for la in (330, 2000):
        for lb in (0, 1, 5):
            for rep in range(3):
                alpha = ACGT if rep else IUPAC
                a = _rand(rng, alpha, la)
                at = int(rng.integers(0, la - 5))
                b = a[at:at + lb].copy() if rep == 1 else _rand(rng, alpha, lb)        # (rep 1: seq_b occurs in seq_a)
                for maxd in (100000, la - lb, la - lb + 1, la + lb):
                    c.add(a, b, 2, maxd, "mode 2")
    for rep in range(4):
        alpha = ACGT if rep % 2 else IUPAC
        b = _rand(rng, alpha, 2000)
        a = _edit(rng, b[:330], alpha, 5 * rep)[:330] if rep < 2 else _rand(rng, alpha, 330)
        if rep == 3:
            a = _high(rng, a, 3)
        for maxd in (100000, 1670, 2330):
            c.add(a, b, 1, maxd, "mode 1")
    return c


# ---- the contexts --------------------------------------------------------------------------------------------------------------
ROUTES = {"default": (), "no_lanes": ("MIA_HIP_MYERS_NO_LANES",), "no_ond": ("MIA_HIP_MYERS_NO_OND",),
          "neither": ("MIA_HIP_MYERS_NO_LANES", "MIA_HIP_MYERS_NO_OND")}


@pytest.fixture(scope="module")
def route():
    """route(name): the context of that name, made once (the switches are read when a context is made)"""
    import mia_amd
    made = {}

    def get(name):
        if name not in made:
            for k in ROUTES[name]:
                os.environ[k] = "1"
            try:
                made[name] = mia_amd.MiaHip(0)
            finally:
                for k in ROUTES[name]:
                    os.environ.pop(k)
        return made[name]

    yield get
    for h in made.values():
        h.close()


def check(got, c, label, want=None):
    want = c.want if want is None else want
    bad = np.nonzero(np.asarray(got) != want)[0]
    rows = [(int(i), int(got[i]), int(want[i]), c.mode[i], c.maxd[i], len(c.A[i]), len(c.B[i])) for i in bad[:8]]
    print("%s: %d pairs, %d wrong (index, got, want, mode, maxd, la, lb) %s" % (label, len(c), len(bad), rows))
    assert len(bad) == 0, (label, len(bad), rows)


# ---- the tests -----------------------------------------------------------------------------------------------------------------
def test_a_lanes(route):
    import mia_amd
    c = lane_cases()
    below, none = int((c.want != NONE).sum()), int((c.want == NONE).sum())
    print("lanes: %d pairs, %d below maxd, %d none" % (len(c), below, none))
    assert below >= 500 and none >= 100
    g = LANE_GROUP
    lb, la = [len(b) for b in c.B[g:g + 64]], [len(a) for a in c.A[g:g + 64]]
    assert {0, 340} <= set(lb) and {0, 320} <= set(la)
    assert any(x == (5, 340, 1) for x in zip(la, lb, c.mode[g:g + 64])) and any(x == (320, 3, 2) for x in zip(la, lb, c.mode[g:g + 64]))
    assert max(len(a) for a in c.A) == 320 and any(max(a) >= 0x80 for a in c.A if a)
    for name in ("default", "no_lanes", "neither"):
        check(route(name).myers(c.A, c.B, c.mode, c.maxd), c, "lanes/" + name)
    check(route("default").myers_packed(mia_amd.pack_myers_pairs(c.A, c.B), c.mode, c.maxd), c, "lanes/packed")
    for lo, hi in ((3, 4), (g - 10, g + 55)):             # a partial last wavefront: 1 pair, 65 pairs
        part = c.take(range(lo, hi))
        check(route("default").myers(part.A, part.B, part.mode, part.maxd), part, "lanes/%d pairs" % (hi - lo), c.want[lo:hi])
        check(route("default").myers_packed(mia_amd.pack_myers_pairs(part.A, part.B), part.mode, part.maxd), part, "lanes/packed %d" % (hi - lo),
              c.want[lo:hi])


def test_b_maxd_edges(route):
    src = [(lane_cases(), range(5, 3008, 15)), (block_cases(), range(0, len(block_cases()), 1)), (cap_cases(), range(0, len(cap_cases()), 30))]
    c = Cases()
    d_of = []
    for cases, idx in src:
        for i in idx:
            d, total = int(cases.dist[i]), len(cases.A[i]) + len(cases.B[i])
            for maxd in (d, d + 1, 0, -1, total, total + 1):
                c.add(cases.A[i], cases.B[i], cases.mode[i], maxd)
                d_of.append(d)
    d_of = np.array(d_of, np.int64)
    n = len(c) // 6
    assert 250 <= n <= 400
    # the programme's answers, and what they must amount to: none at d, 0 and -1; d at d + 1 (unless d is the sum of the lengths,
    # which no maxd admits); at la + lb and beyond, d if it is below the sum
    want = myers_ref.myers_dp(c.A, c.B, c.mode, c.maxd).reshape(n, 6)
    d, total = d_of.reshape(n, 6)[:, 0], np.array([len(a) + len(b) for a, b in zip(c.A[::6], c.B[::6])])
    assert (want[:, [0, 2, 3]] == NONE).all()
    assert (want[d < total, 1] == d[d < total]).all() and (d < total).sum() > 200
    assert (want[:, 4] == want[:, 5]).all() and (want[d < total, 4] == d[d < total]).all()
    for name in ROUTES:
        check(route(name).myers(c.A, c.B, c.mode, c.maxd), c, "maxd/" + name, want.reshape(-1))


def _beyond(c, far):
    """long pairs no D-path cap reaches: unrelated by construction, or a distance above `far`"""
    return int(sum(1 for t, d in zip(c.tag, c.dist) if t == "unrelated" or d > far))


def test_c_one_block_a_lane(route):
    c = block_cases()
    assert 60 <= len(c) <= 70 and 3 * _beyond(c, 800) >= len(c)
    assert {len(a) for a in c.A} == {321, 384, 385, 448, 449, 1024, 1025, 4032, 4033, 4095, 4096} and set(c.mode) == {0, 1, 2}
    assert (c.want != NONE).sum() > 40
    for name in ("default", "no_ond"):
        check(route(name).myers(c.A, c.B, c.mode, c.maxd), c, "blocks/" + name)


def test_d_k_blocks_a_lane_short_seq_b(route):
    import mia_amd
    c = k_short_b_cases()
    assert {len(a) for a in c.A} == set(K_LA) and 3 * _beyond(c, 800) >= len(c)
    assert sum(1 for m, w in zip(c.mode, c.want) if m == 1 and w < 30) >= 5 and (c.want != NONE).sum() > 50
    for name in ("default", "no_ond"):
        check(route(name).myers(c.A, c.B, c.mode, c.maxd), c, "K short/" + name)
    with pytest.raises(mia_amd.MiaHipError):
        route("default").myers([b"A" * 32769], [b"ACGT"], [1], [100])


def test_d_k_blocks_a_lane_long_seq_b(route):
    c = k_long_b_cases()
    short = k_short_b_cases()
    assert 3 * (_beyond(c, 800) + _beyond(short, 800)) >= len(c) + len(short)          # (of all the pairs with K >= 2)
    near = [10 * int(w) < len(a) for t, w, a in zip(c.tag, c.want, c.A) if t != "unrelated"]      # (answered, and close)
    assert all(near) and len(near) == 14
    for name in ("default", "no_ond"):
        check(route(name).myers(c.A, c.B, c.mode, c.maxd), c, "K long/" + name)


def test_e_cap_straddled(route):
    c = cap_cases()
    for la, srange in CAP_RANGES:            # on the programme alone: every row count of the range is somebody's distance
        have = {int(d) for a, d, m in zip(c.A, c.dist, c.mode) if len(a) - (40 if m == 1 else 0) == la}
        assert set(srange) <= have, (la, sorted(set(srange) - have))
    assert any(max(b) >= 0x80 for b in c.B)
    hip = route("default")
    check(hip.myers(c.A, c.B, c.mode, c.maxd), c, "cap/default")
    n = 0
    for i in range(0, len(c), 3):            # (the maxd = 100000 entry of every pair)
        la, s = (int(x) for x in c.tag[i].split("/"))
        if s not in CAP_ALIGN[la]:
            continue
        d, ra, rb = hip.myers_align(c.A[i], c.mode[i], c.B[i], c.maxd[i])
        assert d == int(c.want[i]), (i, d, int(c.want[i]), c.mode[i], la, s)
        ra, rb = ra.encode("latin1"), rb.encode("latin1")
        assert len(ra) == len(rb) and myers_ref.rows_cost(ra, rb) == d, (i, d, c.mode[i], la, s, len(ra), len(rb))
        assert c.A[i].startswith(ra.replace(b"-", b"")) and c.B[i].startswith(rb.replace(b"-", b""))
        n += 1
    assert n == 3 * (5 + 6)


def test_f_second_pair_of_a_workgroup(route):
    c = second_pair_cases()
    assert min(len(a) for a in c.A) > 320 and max(len(a) for a in c.A) <= 400 and max(len(b) for b in c.B) <= 60
    assert len(c) - GRID >= 300
    # (a pair of this size gets a cap of at most sqrt(64 * (60 + 64)) = 89 rows)
    assert 3 * int((c.dist > 200).sum()) >= len(c)
    blocks = lambda p: (len(c.A[p]) + 63) // 64
    seconds = range(GRID, len(c))
    assert sum(1 for q in seconds if blocks(q) < blocks(q - GRID)) >= 300
    done = lambda p: c.mode[p] == 1 and c.maxd[p] > 0 and c.dist[p] < 10        # the D-path kernel finishes it
    on = lambda p: c.mode[p] == 0 and c.maxd[p] > 0 and c.dist[p] > 200        # ... hands it on
    assert sum(1 for q in seconds if on(q - GRID) and done(q)) >= 50 and sum(1 for q in seconds if done(q - GRID) and on(q)) >= 50
    assert sum(1 for q in seconds if c.maxd[q - GRID] <= 0) >= 30 and sum(1 for q in seconds if c.maxd[q] <= 0) >= 30
    assert sum(1 for q in seconds if not c.B[q - GRID]) >= 30 and sum(1 for q in seconds if not c.B[q]) >= 30
    assert (c.want != NONE).sum() > 3000 and (c.want == NONE).sum() > 300
    for name in ("default", "no_ond"):
        check(route(name).myers(c.A, c.B, c.mode, c.maxd), c, "second pair/" + name)


def test_g_beyond_the_lds_budget(route):
    c = lds_cases()
    assert c.want[1] > 309_000 and c.want[0] < 250 and c.want[0] == c.want[2] and c.want[3] < 100 and c.want[4] < 30
    hip = route("default")
    one = c.take([0])
    check(hip.myers(one.A, one.B, one.mode, one.maxd), one, "lds/alone", c.want[:1])
    rest = c.take(range(1, 5))
    check(hip.myers(rest.A, rest.B, rest.mode, rest.maxd), rest, "lds/beside others", c.want[1:])


def test_h_other_side_far_shorter(route):
    c = short_side_cases()
    assert (c.want != NONE).sum() >= 30 and (c.want == NONE).sum() >= 10 and any(max(a) >= 0x80 for a in c.A)
    for name in ("default", "no_ond"):
        check(route(name).myers(c.A, c.B, c.mode, c.maxd), c, "short side/" + name)
