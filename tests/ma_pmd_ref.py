"""The damage score of ma_hip (-L, -K, -S, -f 97) restated in Python over a maln_synth.Maln, from the text of DESIGN.md ("Damage
score"): a loop over records and columns and a dictionary of molecules.  Nothing here is shared with the kernels or with
csrc/ma_pmd_body.h.  The rule stands on the substitution profile's, so a column's event is taken from that rule's own restatement
(tests/ma_profile_ref.py, event): ("beyond",), ("bad_code",), ("del", d') or ("count", d', i', j'), already in the read's orientation.

  a weight table w[31][5][5] (int32, units of 2^-16 nat); a record's score = the sum of w[d'][i'][j'] over its count events, 0 for a
  record with use == 0; molecules as for -u (mate: -1, -2 or the other half); S = the sum of the records' scores; the strand is that of
  the lowest-numbered record; a molecule counts if one of its records has use != 0; keep = S >= threshold;
  hist[strand][clamp(floor(S / 32768) + 20, 0, 63)] over the molecules that count
"""
import math

import numpy as np

import ma_dedup_ref
import ma_profile_ref

A, C, G, T = 0, 1, 2, 3
UNIT = 65536
DEFAULTS = (0.3, 0.01, 0.001, 0.001 / 3)
MAX_WEIGHT = 1 << 20


def model_table(p=DEFAULTS[0], c0=DEFAULTS[1], pi=DEFAULTS[2], eps=DEFAULTS[3], ss=False):
    """w[31, 5, 5] of the model; None where the parameters are refused"""
    if not all(math.isfinite(x) for x in (p, c0, pi, eps)) or not (0 < p < 1 and 0 <= c0 < 1 and 0 < pi < 1 and 0 < eps < 1):
        return None

    def g(k):
        return p * (1 - p) ** (k - 1)

    def like(D):
        return (1 - pi) * (1 - eps) * (1 - D) + (1 - pi) * eps * D + pi * eps * (1 - D)

    def q(x):
        return math.floor(x * UNIT + 0.5)

    w = np.zeros((31, 5, 5), np.int64)
    for d in range(31):
        g5 = g(d + 1) if d <= 14 else 0.0
        g3 = g(31 - d) if d >= 16 else 0.0
        d_ct = c0 + g5 + (g3 if ss else 0.0)
        d_ga = c0 + g3
        if d_ct >= 1 or d_ga >= 1:
            return None
        w[d, C, C] = q(math.log(like(d_ct) / like(0.0)))
        w[d, C, T] = q(math.log((1 - like(d_ct)) / (1 - like(0.0))))
        if not ss:
            w[d, G, G] = q(math.log(like(d_ga) / like(0.0)))
            w[d, G, A] = q(math.log((1 - like(d_ga)) / (1 - like(0.0))))
    return w


def events(m):
    """per record the (d', i', j') of its count events, a row each: the loop over records and columns, made once per file"""
    out = []
    for rec in m.rec:
        rows = []
        for c in range(rec["end"] - rec["start"] + 1):
            e = ma_profile_ref.event(m.L, m.ref_seq, rec["start"], c, rec["seq"][c], rec["smp"][c], bool(rec["rc"]))
            if e[0] == "count":
                rows.append(e[1:])
        out.append(np.array(rows, np.int64).reshape(len(rows), 3))
    return out


def record_scores(m, w, use=None, ev=None):
    """rec_score[n]: the weights of a record's events added up in int64 (775 weights of at most 2^20 each: no sum leaves it)"""
    ev = events(m) if ev is None else ev
    w = np.asarray(w, np.int64)
    return np.array([int(w[e[:, 0], e[:, 1], e[:, 2]].sum()) if use is None or use[r] else 0 for r, e in enumerate(ev)], np.int64).reshape(len(ev))


def bin_of(S):
    return min(max(S // 32768 + 20, 0), 63)                  # (Python's // is the floor division)


def score(m, w, threshold, use=None, mate=None, rec=None, ev=None):
    """(rec_score, mol_score, keep, hist[2, 64], n_molecules, n_kept, orphans)"""
    n = len(m.rec)
    mate = ma_dedup_ref.pair_halves(m.rec) if mate is None else mate
    rec = record_scores(m, w, use, ev) if rec is None else rec
    molecules = {}                                           # lowest record number -> its records
    for r in range(n):
        molecules.setdefault(min(r, int(mate[r])) if mate[r] >= 0 else r, []).append(r)
    mol, keep, hist, orphans = np.zeros(n, np.int64), np.zeros(n, np.uint8), np.zeros((2, 64), np.int64), 0
    for first, recs in molecules.items():
        S = sum(int(rec[r]) for r in recs)
        for r in recs:
            mol[r] = S
            keep[r] = 1 if S >= threshold else 0
        if use is None or any(use[r] for r in recs):
            hist[1 if m.rec[first]["rc"] else 0, bin_of(S)] += 1
            orphans += 1 if mate[first] == -2 else 0
    return rec, mol, keep, hist, int(hist.sum()), int(keep.sum()), orphans


def threshold_of(nat):
    return math.floor(nat * UNIT + 0.5)


def table_of(hist, orphans, n_used, ss, params=DEFAULTS):
    """-f 97 from hist alone"""
    out = ["# ma_hip damage scores: %d molecules, %d orphan halves, %d records, library %s, p %g c0 %g pi %g eps %g\n" %
           ((int(hist.sum()), orphans, n_used, "ss" if ss else "ds") + tuple(params)),
           "# from\t+\t-\tall\tfrom+\tfrom-\tfrom_all\n"]
    for b in range(64):
        rows = (hist[0], hist[1], hist[0] + hist[1])
        out.append("\t".join(["-inf" if b == 0 else "%.1f" % ((b - 20) / 2)] + [str(int(h[b])) for h in rows] + [str(int(h[b:].sum())) for h in rows]) + "\n")
    return "".join(out)


def table(m, w, use_dropped=False, ss=False, params=DEFAULTS):
    """-f 97 of a file"""
    use = None if use_dropped else np.array([0 if r["dr"] else 1 for r in m.rec], np.uint8)
    hist, orphans = score(m, w, 0, use)[3::3]
    return table_of(hist, orphans, len(m.rec) if use is None else int(use.sum()), ss, params)


def reduce(m, keep):
    """the Maln without the records that are not kept, GAPS reset as for -u"""
    return ma_dedup_ref.reduce(m, keep)
