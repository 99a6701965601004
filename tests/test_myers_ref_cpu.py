"""tests/myers_ref.py -- the plain dynamic programme the GPU Myers tests hold the kernels to -- is itself pinned: to the REAL
reference's myers_diff answers (tests/golden/myers_vectors.txt, every pair of it), to the oracle's D-path search
(oracle/mia_oracle.c: ora_myers_diff) on random pairs of every shape the programme treats differently (an empty side, a side of
a few characters, maxd at the distance itself), and to the CPU emulation of the D-path kernel's body.  CPU only."""
import os

import numpy as np

import myers_ref
from conftest import GOLDEN
from test_emul_myers_ond import emu, long_pairs, run  # noqa: F401  (emu: the fixture that builds the emulation)


def test_every_golden_vector():
    lines = [l.rstrip("\n") for l in open(os.path.join(GOLDEN, "myers_vectors.txt"))]
    A, B, mode, maxd, exp = [], [], [], [], []
    for inp, out in zip(lines[0::2], lines[1::2]):
        m, d, a, b = inp.split(" ")
        A.append(a.encode()); B.append(b.encode()); mode.append(int(m)); maxd.append(int(d)); exp.append(int(out.split(" ")[0]))
    got = myers_ref.myers_dp(A, B, mode, maxd)
    bad = [(i, int(got[i]), exp[i], mode[i], maxd[i], len(A[i]), len(B[i])) for i in range(len(exp)) if int(got[i]) != exp[i]]
    assert not bad, bad[:10]
    assert len(exp) >= 221 and max(len(a) for a in A) > 16_000


def random_pairs(n=2400, seed=31):
    """(seq_a, seq_b, mode) -- the alphabet of test_lane_kernel_equals_systolic_kernel: unrelated pairs, edited copies, overhangs,
    an empty side, one side of 1..5 characters against 300 or more"""
    rng = np.random.default_rng(seed)
    alpha = np.frombuffer(b"ACGTACGTACGTNRYKMSWBDHVacgtnX-", np.uint8)
    rand = lambda k: alpha[rng.integers(0, len(alpha), k)].copy()
    A, B, mode = [], [], []
    for i in range(n):
        kind = i % 8
        la = int(rng.integers(0, 401))
        a = rand(la)
        if kind == 0:
            b = rand(int(rng.integers(0, 401)))
        elif kind == 1:
            a, b = (rand(0), rand(int(rng.integers(0, 401)))) if i % 16 == 1 else (a, rand(0))
        elif kind == 2:
            short, long_ = rand(int(rng.integers(1, 6))), rand(int(rng.integers(300, 401)))
            if i % 16 == 2:
                long_[int(rng.integers(0, len(long_) - 5)):][:len(short)] = short          # the short side occurs in the long one
            a, b = (short, long_) if (i // 8) % 2 else (long_, short)
        else:
            b = list(a)
            for _ in range(int(rng.integers(0, 1 + la // (3 if kind == 3 else 12)))):
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
            if kind == 4 and len(b) > 20:
                b = b[int(rng.integers(0, 10)):len(b) - int(rng.integers(0, 10))]
            b = np.array(b[:400], np.uint8)
        A.append(a.tobytes()); B.append(b.tobytes()); mode.append(int(rng.integers(0, 3)))
    return A, B, mode


def test_oracle_dpath_search_on_random_pairs(oracle):
    A, B, mode = random_pairs()
    d = myers_ref.myers_distance(A, B, mode)
    rng = np.random.default_rng(32)
    maxd = np.stack([rng.choice([1, 2, 5, 30, 100000], len(A)), d, d + 1], 1)          # three calls per pair
    got = myers_ref.myers_dp(np.repeat(np.array(A, object), 3), np.repeat(np.array(B, object), 3), np.repeat(mode, 3), maxd.reshape(-1)).reshape(-1, 3)
    n_none = n_some = n_empty = n_tiny = 0
    for i, (a, b, m) in enumerate(zip(A, B, mode)):
        for k in range(3):
            want = oracle.ora_myers_diff(a, m, b, int(maxd[i, k]), None)
            assert int(got[i, k]) == want, (i, int(got[i, k]), want, m, int(maxd[i, k]), len(a), len(b))
            n_none += want == 0xFFFFFFFF
            n_some += want != 0xFFFFFFFF
        n_empty += min(len(a), len(b)) == 0
        n_tiny += 1 <= min(len(a), len(b)) <= 5 and max(len(a), len(b)) >= 300
    assert len(A) >= 2000 and n_none > 2000 and n_some > 2000 and n_empty > 200 and n_tiny > 200


def test_emulated_dpath_body_on_long_pairs(emu):  # noqa: F811
    pairs = long_pairs()
    want = myers_ref.myers_dp([a for _, a, _ in pairs], [b for _, _, b in pairs], [m for m, _, _ in pairs], [100000] * len(pairs))
    for it, (mode, a, b) in enumerate(pairs):
        d, _ra, _rb = run(emu, a, mode, b, 100000, 1 << 20)
        assert d == int(want[it]), (it, mode, len(a), len(b))
    assert (want < 200).all()


def test_rows_cost():
    assert myers_ref.rows_cost("AC-GT", "ANTGX") == 2          # a gap, and X meets nothing (not even itself)
    assert myers_ref.rows_cost(b"acgu", b"ACGT") == 0
    assert myers_ref.rows_cost("X-", "X-") == 2
