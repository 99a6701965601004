"""The duplicate filter (ma_hip -u, -t) restated from DESIGN.md, "Duplicate filter": plain Python, a sort and a serial walk, as
the reference's sort_fsdb + set_uniq_in_fsdb (just_outer_coords, tolerance) do it.  Nothing here is shared with the kernels or with
csrc/ma_dedup_body.h: no keys, no mirroring, no scans.

Records are maln_synth's dicts (id, seg, rc, start, end, score, ins) in FILE order."""
import copy

import numpy as np

SIZES = 1025


def pair_halves(recs):
    """mate per record: -1 a molecule of its own, -2 an orphan half, else the record number of the other half"""
    n = len(recs)
    mate = np.full(n, -1, np.int64)
    stems = {}
    for i, r in enumerate(recs):
        if r["seg"] not in ("f", "b"):
            continue
        mate[i] = -2
        if r["id"].endswith("_" + r["seg"]):
            stems.setdefault((1 if r["rc"] else 0, r["id"][:-1]), {"f": [], "b": []})[r["seg"]].append(i)
    for lists in stems.values():
        if len(lists["f"]) == 1 and len(lists["b"]) == 1:
            f, b = lists["f"][0], lists["b"][0]
            mate[f], mate[b] = b, f
    return mate


def molecules(recs, L, mate):
    """[(rc, a, e, score, index, records)] and the orphans' record numbers"""
    mols, orphans = [], []
    for i, r in enumerate(recs):
        if mate[i] == -2:
            orphans.append(i)
        elif mate[i] == -1:
            mols.append((1 if r["rc"] else 0, r["start"], r["end"], r["score"], i, (i,)))
        elif r["seg"] == "f":
            b = int(mate[i])
            mols.append((1 if r["rc"] else 0, r["start"], recs[b]["end"] + L, r["score"], min(i, b), (i, b)))
    return mols, orphans


def dedup(recs, L, t=0, mate=None):
    """(keep, rep, hist[2, 1025], n_molecules, n_clusters, orphans)"""
    assert 0 <= t <= 100
    n = len(recs)
    mate = pair_halves(recs) if mate is None else mate
    mols, orphans = molecules(recs, L, mate)
    keep, rep, hist = np.zeros(n, np.uint8), np.zeros(n, np.int64), np.zeros((2, SIZES), np.int64)
    for i in orphans:
        keep[i], rep[i] = 1, i
    # fs_comp: reverse first; forward by a up, e down; reverse by e down, a up.  Within equal coordinates: score down, index up.
    mols.sort(key=lambda m: (0, -m[2], m[1], -m[3], m[4]) if m[0] else (1, m[1], -m[2], -m[3], m[4]))
    clusters = []                                           # [representative molecule, strand, [molecules]]
    anchor = None
    for m in mols:
        coords = (m[0], m[1], m[2])
        if anchor is not None and coords == anchor_run:
            clusters[-1][2].append(m)                       # the anchor's own run, or a duplicate run met again: same cluster
        elif anchor is not None and m[0] == anchor[0] and abs(m[1] - anchor[1]) <= t and abs(m[2] - anchor[2]) <= t:
            clusters[-1][2].append(m)
            anchor_run = coords
        else:
            anchor = anchor_run = coords
            clusters.append([m, m[0], [m]])                 # first of its run in the sort: the run's best
    for best, rc, members in clusters:
        hist[rc, min(len(members), SIZES - 1)] += 1
        for m in members:
            for r in m[5]:
                rep[r] = best[4]
                keep[r] = 1 if m is best else 0
    return keep, rep, hist, len(mols), len(clusters), len(orphans)


def group_by(recs, L, mate=None):
    """t = 0 as a plain group-by on (rc, a, e): {coordinates: [molecules]}"""
    mate = pair_halves(recs) if mate is None else mate
    groups = {}
    for m in molecules(recs, L, mate)[0]:
        groups.setdefault((m[0], m[1], m[2]), []).append(m)
    return groups


def device_arrays(recs, mate=None):
    """(start, end, revcom, score, mate) as MiaHip.ma_dedup takes them"""
    mate = pair_halves(recs) if mate is None else mate
    return (np.array([r["start"] for r in recs], np.int32), np.array([r["end"] for r in recs], np.int32),
            np.array([1 if r["rc"] else 0 for r in recs], np.uint8), np.array([r["score"] for r in recs], np.int32), mate)


def new_gaps(m, keep):
    """GAPS after the records with keep == 0 are gone (cull_maln_from_fsdb): only columns with GAPS > 0 change, to the longest insert
    a kept record with START < i <= END carries at i - START -- the last pair given for that position -- or 0"""
    longest = np.zeros(m.L, np.int64)
    for r, k in zip(m.rec, keep):
        if not k:
            continue
        at = {}
        for pos, text in r["ins"]:
            at[pos] = text
        for pos, text in at.items():
            i = r["start"] + pos
            if r["start"] < i <= r["end"] and i < m.L:
                longest[i] = max(longest[i], len(text))
    return np.where(m.gaps > 0, longest, m.gaps).astype(np.int32)


def reduce(m, keep):
    """the Maln without the records that are not kept, GAPS recomputed; everything else as it was"""
    out = copy.copy(m)
    out.rec = [r for r, k in zip(m.rec, keep) if k]
    out.gaps = new_gaps(m, keep)
    return out

