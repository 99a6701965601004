"""The plain dynamic programme the Myers kernels are held to (TEST INFRASTRUCTURE; imports nothing from mia_amd).

The definition is the one in the header of csrc/mia_myers_kernels.h: unit costs, two characters match when their IUPAC
bitmaps (src/myers_align.h:40-67) intersect,

    D[i][0] = i,  D[0][j] = j,
    D[i][j] = min(D[i-1][j-1] + (bits(a[i-1]) & bits(b[j-1]) == 0), D[i-1][j] + 1, D[i][j-1] + 1)

    mode 0   D[la][lb]
    mode 1   min_i D[i][lb]      (all of seq_b, a prefix of seq_a)
    mode 2   min_j D[la][j]      (all of seq_a, a prefix of seq_b)

and the answer is d if d < min(maxd, la + lb), else 0xFFFFFFFF (so maxd <= 0 admits nothing).

The programme runs row by row in numpy, many pairs side by side: the rows follow the shorter sequence of a pair, the
longer one lies along the vector, and the dependency inside a row, D[i][j] = min(t[j], D[i][j-1] + 1), is the running
minimum of t[j] - j, plus j.  A pair is computed once for all three modes."""
import numpy as np

NONE = 0xFFFFFFFF

BITS = np.zeros(256, np.uint8)
for _c, _v in zip(b"ACGTUSWRYKMBDHVN", (1, 2, 4, 8, 8, 6, 9, 5, 10, 12, 3, 14, 13, 11, 7, 15)):
    BITS[_c] = _v
    BITS[_c | 32] = _v              # case-insensitive; every other byte (X, -, 0x80..0xFF) is compatible with nothing

_BATCH_CELLS = 1 << 20              # cells of one row of a batch (pairs x padded length): what is worked on at a time


def _bytes(s):
    return s if isinstance(s, (bytes, bytearray)) else s.encode("latin1")


def _batch(rows, cols):
    """rows, cols: lists of uint8 bitmap arrays (one pair each; the programme's rows follow `rows`).
    Returns int64 arrays (D[lr][lc], min_i D[i][lc], min_j D[lr][j])."""
    P = len(rows)
    lr = np.array([len(r) for r in rows], np.int64)
    lc = np.array([len(c) for c in cols], np.int64)
    order = np.argsort(lr, kind="stable")           # a pair leaves the batch when its last row is done
    lr, lc = lr[order], lc[order]
    R, W = int(lr.max()), int(lc.max())
    br = np.zeros((P, max(R, 1)), np.uint8)
    bc = np.zeros((P, W), np.uint8)
    for n, p in enumerate(order):
        br[n, :lr[n]] = rows[p]
        bc[n, :lc[n]] = cols[p]
    ar = np.arange(W + 1, dtype=np.int32)
    D = np.tile(ar, (P, 1))                         # row 0: D[0][j] = j
    T = np.empty_like(D)
    U = np.empty((P, W), np.int32)
    pidx = np.arange(P)
    last = lc.copy()                                # D[lr][lc]; for lr = 0 that is row 0
    colmin = lc.copy()                              # min_i D[i][lc], i = 0 counted
    rowmin = np.zeros(P, np.int64)                  # min_j D[lr][j]; for lr = 0 that is D[0][0] = 0
    inside = ar[None, :] <= lc[:, None]
    for i in range(1, R + 1):
        s = int(np.searchsorted(lr, i))             # pairs s.. still have a row i
        d, t, u = D[s:], T[s:], U[s:]
        np.add(d[:, :-1], (bc[s:] & br[s:, i - 1, None]) == 0, out=t[:, 1:])     # diagonal step
        np.add(d[:, 1:], 1, out=u)                                               # a character of `rows` alone
        np.minimum(t[:, 1:], u, out=t[:, 1:])
        t[:, 0] = i
        t -= ar
        np.minimum.accumulate(t, axis=1, out=t)                                  # a character of `cols` alone
        t += ar
        D, T = T, D
        v = t[pidx[:P - s], lc[s:]]
        colmin[s:] = np.minimum(colmin[s:], v)
        e = int(np.searchsorted(lr, i, side="right"))      # pairs s..e-1 end with this row
        if e > s:
            last[s:e] = v[:e - s]
            rowmin[s:e] = np.where(inside[s:e], t[:e - s], np.int32(2**31 - 1)).min(axis=1)
    out = [np.empty(P, np.int64) for _ in range(3)]
    for o, src in zip(out, (last, colmin, rowmin)):
        o[order] = src
    return out


def myers_distances(pairs):
    """pairs: list of (seq_a, seq_b) as bytes.  Returns an int64 array [n, 3]: the distance of every pair in modes 0, 1, 2,
    before maxd is applied."""
    n = len(pairs)
    out = np.zeros((n, 3), np.int64)
    if n == 0:
        return out
    rows, cols, swapped = [], [], np.zeros(n, bool)
    for p, (a, b) in enumerate(pairs):
        ba, bb = BITS[np.frombuffer(_bytes(a), np.uint8)], BITS[np.frombuffer(_bytes(b), np.uint8)]
        if len(ba) <= len(bb):
            rows.append(ba); cols.append(bb)        # rows over seq_a: min_i D[i][lb] is mode 1, min_j D[la][j] mode 2
        else:
            rows.append(bb); cols.append(ba); swapped[p] = True      # the transposed pair: modes 1 and 2 change places
    lc = np.array([len(c) for c in cols], np.int64)
    order = np.argsort(lc, kind="stable")
    k = 0
    while k < n:                                    # batches of pairs of about the same length along the vector
        first = int(lc[order[k]])
        e = k + 1
        while e < n and lc[order[e]] <= first + first // 4 + 32 and (e - k + 1) * (int(lc[order[e]]) + 1) <= _BATCH_CELLS:
            e += 1
        idx = order[k:e]
        g, cm, rm = _batch([rows[p] for p in idx], [cols[p] for p in idx])
        out[idx, 0] = g
        out[idx, 1] = np.where(swapped[idx], rm, cm)
        out[idx, 2] = np.where(swapped[idx], cm, rm)
        k = e
    return out


def myers_distance(seq_a, seq_b, mode):
    """int64[n]: the distances before maxd is applied (every distinct pair is computed once, whatever its modes)"""
    keys = {}
    which = np.empty(len(seq_a), np.int64)
    for p, (a, b) in enumerate(zip(seq_a, seq_b)):
        which[p] = keys.setdefault((_bytes(a), _bytes(b)), len(keys))
    d3 = myers_distances(list(keys))
    return d3[which, np.asarray(mode, np.int64)] if len(which) else np.zeros(0, np.int64)


def myers_dp(seq_a, seq_b, mode, maxd):
    """np.uint32[n]: what mia_hip_myers must answer for these pairs"""
    d = myers_distance(seq_a, seq_b, mode)
    total = np.array([len(_bytes(a)) + len(_bytes(b)) for a, b in zip(seq_a, seq_b)], np.int64)
    limit = np.minimum(np.asarray(maxd, np.int64), total)
    return np.where(d < limit, d, NONE).astype(np.uint32)


def rows_cost(row_a, row_b):
    """the cost of two alignment rows of equal length: columns with a gap, or with two characters whose bitmaps do not meet"""
    ra, rb = np.frombuffer(_bytes(row_a), np.uint8), np.frombuffer(_bytes(row_b), np.uint8)
    assert len(ra) == len(rb)
    return int(((ra == 45) | (rb == 45) | ((BITS[ra] & BITS[rb]) == 0)).sum())
