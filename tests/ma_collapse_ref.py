"""The duplicate consensus (ma_hip -u -j, -f 98; MiaHip.ma_collapse) restated from DESIGN.md, "Duplicate consensus": plain Python loops
over clusters, records and columns.  The clusters, their representative and keep come from ma_dedup_ref.dedup; nothing else is shared
with anything, and nothing at all with the kernels or csrc/ma_collapse_body.h: no chunks, no count array, no voter words.

Records are maln_synth's dicts in FILE order; vote holds one entry per record (None: everyone votes; ma_hip passes not DR)."""
import copy

import numpy as np

import ma_dedup_ref as dd

CLASSES = "ACGT-"
SIZE_BINS = ("2", "3", "4", "5-8", "9-16", "17+")
CLUSTERS, COLUMNS, SPLIT, TO_BASE, TO_GAP, TO_N = range(6)
MAX_INPUTS = 2 ** 31 - 1


def size_bin(members):
    assert members >= 2
    return members - 2 if members <= 4 else 3 if members <= 8 else 4 if members <= 16 else 5


def decide(counts, own, edge):
    """(new character, voted, split, what) for one column: counts = {class: votes}, what = None or TO_BASE / TO_GAP / TO_N"""
    counts = {k: v for k, v in counts.items() if v > 0 and not (edge and k == "-")}
    if not counts:
        return own, False, False, None
    top = max(counts.values())
    ahead = [k for k in CLASSES if counts.get(k, 0) == top]
    split = len(counts) > 1
    if len(ahead) == 1:
        if ahead[0] == own.upper():
            return own, True, split, None
        return ahead[0], True, split, TO_GAP if ahead[0] == "-" else TO_BASE
    if own.upper() in ahead or own == "N":                  # (a tie over an N leaves the byte: nothing changed)
        return own, True, split, None
    return "N", True, split, TO_N


def clusters_of(recs, L, t, mate=None):
    """(keep, rep, [(representative molecule, [molecules])], totals): molecules as ma_dedup_ref.molecules gives them"""
    mate = dd.pair_halves(recs) if mate is None else mate
    keep, rep, _hist, n_mol, n_clu, orphans = dd.dedup(recs, L, t, mate)
    by_rep = {}
    for mol in dd.molecules(recs, L, mate)[0]:
        by_rep.setdefault(int(rep[mol[5][0]]), []).append(mol)
    out = []
    for idx, mols in by_rep.items():
        best = [mol for mol in mols if mol[4] == idx]
        assert len(best) == 1
        out.append((best[0], mols))
    return keep, rep, out, (n_mol, n_clu, orphans)


def vote_at(recs, mol, p):
    """the character the molecule casts at reference column p: its whole or front record first, then its back half; None for none"""
    for q in mol[5]:
        r = recs[q]
        if r["start"] <= p <= r["end"]:
            return r["seq"][p - r["start"]]
    return None


def collapse_records(m, t=0, vote=None):
    """(records with SEQ and NUM_INPUTS rewritten -- all of them, in file order --, keep, members, hist[2, 6, 6], n_collapsed, n_changed,
    totals of the filter)"""
    recs = m.rec
    keep, _rep, clusters, totals = clusters_of(recs, m.L, t)
    out = [dict(r) for r in recs]
    members, hist = np.zeros(len(recs), np.int32), np.zeros((2, 6, 6), np.int64)
    for best, mols in clusters:
        if len(mols) < 2:
            continue
        row = hist[best[0], size_bin(len(mols))]
        row[CLUSTERS] += 1
        voters = [mol for mol in mols if vote is None or vote[mol[5][0]]]
        inputs = min(sum(1 if recs[mol[5][0]]["num_inputs"] is None else recs[mol[5][0]]["num_inputs"] for mol in voters), MAX_INPUTS)     # (no NUM_INPUTS line reads as 1)
        for R in best[5]:
            r = recs[R]
            members[R] = len(mols)
            n = r["end"] - r["start"] + 1
            seq = list(r["seq"])
            for c in range(n):
                counts = {}
                for mol in voters:
                    ch = vote_at(recs, mol, r["start"] + c)
                    if ch is not None and ch.upper() in CLASSES:
                        counts[ch.upper()] = counts.get(ch.upper(), 0) + 1
                seq[c], voted, split, what = decide(counts, seq[c], c == 0 or c == n - 1)
                row[COLUMNS] += voted
                row[SPLIT] += split
                if what is not None:
                    row[what] += 1
            out[R]["seq"] = "".join(seq)
            if voters:
                out[R]["num_inputs"] = inputs
    return out, keep, members, hist, int(hist[:, :, CLUSTERS].sum()), int(hist[:, :, TO_BASE:].sum()), totals


def collapse(m, t=0, vote=None):
    """(the new Maln: the kept records rewritten, GAPS as under -u; members; hist)"""
    out, keep, members, hist = collapse_records(m, t, vote)[:4]
    full = copy.copy(m)
    full.rec = out
    return dd.reduce(full, keep), members, hist


def not_dropped(m):
    """the vote ma_hip passes: a dropped copy does not vote"""
    return np.array([0 if r["dr"] else 1 for r in m.rec], np.uint8)


def report(m, t=0, vote=None):
    """the text of ma_hip -u -j [-t N] -f 98"""
    _o, _k, _m, hist, collapsed, _c, (n_mol, n_clu, orphans) = collapse_records(m, t, vote)
    out = ["# ma_hip duplicate consensus: %d molecules, %d clusters, %d collapsed, %d orphans, tolerance %d\n" % (n_mol, n_clu, collapsed, orphans, t),
           "# size\tstrand\tclusters\tcolumns\tsplit\tto_base\tto_gap\tto_N\n"]
    for b, label in enumerate(SIZE_BINS):
        for strand in (0, 1):
            out.append("%s\t%s\t%s\n" % (label, "-" if strand else "+", "\t".join(str(int(x)) for x in hist[strand, b])))
    return "".join(out)
