"""The deaminated-fragment filter of ma_hip (-D, -e, -S, -f 95) restated in Python over a maln_synth.Maln, from the text of DESIGN.md
("Deaminated fragments"): a loop over records and columns and a dictionary of molecules.  Nothing here is shared with the kernels or
with csrc/ma_damage_body.h.  The rule stands on the substitution profile's, so a column's event is taken from that rule's own
restatement (tests/ma_profile_ref.py, event): ("beyond",), ("bad_code",), ("del", d') or ("count", d', i', j'), already in the
read's orientation.

  a 5' hit at k = 1 .. 15: ("count", k - 1, C, T)
  a 3' hit at k = 1 .. 15: ("count", 31 - k, G, A) for a double-stranded library, ("count", 31 - k, C, T) for a single-stranded one
  a record with use == 0 yields no hits; pos5 / pos3 of a record = its smallest k, 0 for none
  molecules as for -u (mate: -1, -2 or the other half); m5 / m3 = the smallest non-zero pos5 / pos3 of its records; its strand is that
  of its lowest-numbered record; it counts if one of its records has use != 0
"""
import numpy as np

import ma_dedup_ref
import ma_profile_ref

A, C, G, T = 0, 1, 2, 3
MODES = ("any", "5", "3", "both")
GRID_N = (1, 2, 3, 15)


def hits(m, use=None, ss=False):
    """every hit as (record, end, k), end "5" or "3" (for tests only)"""
    out = []
    for r, rec in enumerate(m.rec):
        if use is not None and not use[r]:
            continue
        for c in range(rec["end"] - rec["start"] + 1):
            e = ma_profile_ref.event(m.L, m.ref_seq, rec["start"], c, rec["seq"][c], rec["smp"][c], bool(rec["rc"]))
            if e[0] != "count":
                continue
            _, d, i, j = e
            if d <= 14 and (i, j) == (C, T):
                out.append((r, "5", d + 1))
            if d >= 16 and (i, j) == ((C, T) if ss else (G, A)):
                out.append((r, "3", 31 - d))
    return out


def positions(m, use=None, ss=False, found=None):
    """(pos5[n], pos3[n])"""
    n = len(m.rec)
    pos = {"5": np.zeros(n, np.uint8), "3": np.zeros(n, np.uint8)}
    for r, end, k in (hits(m, use, ss) if found is None else found):
        if pos[end][r] == 0 or k < pos[end][r]:
            pos[end][r] = k
    return pos["5"], pos["3"]


def kept(m5, m3, n_pos, mode):
    k5, k3 = 0 < m5 <= n_pos, 0 < m3 <= n_pos
    return {"5": k5, "3": k3, "any": k5 or k3, "both": k5 and k3}[mode]


def damage(m, n_pos, mode="any", ss=False, use=None, mate=None, pos=None):
    """(pos5, pos3, keep, hist[2, 16, 16], n_molecules, n_kept, orphans)"""
    assert 1 <= n_pos <= 15 and mode in MODES
    n = len(m.rec)
    mate = ma_dedup_ref.pair_halves(m.rec) if mate is None else mate
    pos5, pos3 = positions(m, use, ss) if pos is None else pos
    molecules = {}                                           # lowest record number -> its records
    for r in range(n):
        molecules.setdefault(min(r, int(mate[r])) if mate[r] >= 0 else r, []).append(r)
    keep, hist, orphans = np.zeros(n, np.uint8), np.zeros((2, 16, 16), np.int64), 0
    for first, recs in molecules.items():
        m5 = min([int(pos5[r]) for r in recs if pos5[r]] or [0])
        m3 = min([int(pos3[r]) for r in recs if pos3[r]] or [0])
        for r in recs:
            keep[r] = 1 if kept(m5, m3, n_pos, mode) else 0
        if use is None or any(use[r] for r in recs):
            hist[1 if m.rec[first]["rc"] else 0, m5, m3] += 1
            orphans += 1 if mate[first] == -2 else 0
    return pos5, pos3, keep, hist, int(hist.sum()), int(keep.sum()), orphans


def table_of(hist, orphans, n_used, ss):
    """-f 95 from hist alone"""
    out = ["# ma_hip damage classes: %d molecules, %d orphan halves, %d records, library %s\n" % (int(hist.sum()), orphans, n_used, "ss" if ss else "ds"),
           "# N" + "".join("\t%s%s" % (what, strand) for strand in ("+", "-", "") for what in ("5p", "3p", "both", "either")) + "\n"]
    for n_pos in range(1, 16):
        row = [str(n_pos)]
        for h in (hist[0], hist[1], hist[0] + hist[1]):
            k5, k3 = h[1:n_pos + 1, :].sum(), h[:, 1:n_pos + 1].sum()
            both = h[1:n_pos + 1, 1:n_pos + 1].sum()
            row += [str(int(x)) for x in (k5, k3, both, k5 + k3 - both)]
        out.append("\t".join(row) + "\n")
    return "".join(out)


def table(m, use_dropped=False, ss=False):
    """-f 95 of a file"""
    use = None if use_dropped else np.array([0 if r["dr"] else 1 for r in m.rec], np.uint8)
    _p5, _p3, _keep, hist, _n, _k, orphans = damage(m, 15, "any", ss, use)
    return table_of(hist, orphans, len(m.rec) if use is None else int(use.sum()), ss)


def reduce(m, keep):
    """the Maln without the records that are not kept, GAPS reset as for -u"""
    return ma_dedup_ref.reduce(m, keep)
