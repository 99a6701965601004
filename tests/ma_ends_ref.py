"""Fragment-end context (ma_hip -f 92) and read lengths (-f 93) restated in Python over a maln_synth.Maln.  The reference's `ma` has
neither report; the rule below is the project's own ("Fragment ends and read lengths") and is written here from its
text, not from csrc/ma_ends_body.h.  Two places tie it to what the reference does produce: which record ends are real, and on which
strand, is what its format 3 counts in columns 5-8 (true_ends below); a read's length is the length of the SEQ field of the SAM
export (tests/ma_sam_ref.py).

A record: s = START, n its columns, e = s + n - 1, rc, seg = the SEG character, d = +1 for rc == 0 and -1 for rc == 1.  Every record
is stored in reference orientation.  A record marked DR is left out unless dropped records are asked for.
True ends (a read split at the origin is two records, a front one 'f' and a back one 'b'):
              rc == 0                    rc == 1
  5' end      a = s, if seg != 'b'       a = e, if seg != 'f'
  3' end      a = e, if seg != 'f'       a = s, if seg != 'b'
Positions k = -10 .. -1 and +1 .. +10; no position 0.
  5' end: k > 0 is inside the read, column a + d (k - 1); k < 0 in front of it, column a + d k.
  3' end: k < 0 is inside (-1 the read's last base), column a + d (k + 1); k > 0 behind it, column a + d k.
Class of column p: 5 when p is not in 0 .. L-1 (no wrap); else upper(ref_seq[p]) A C G T -> 0 1 2 3, anything else 4; for rc == 1 a
class c < 4 becomes 3 - c.  Each event adds one to ctx[end][o][class], end 0 = 5', 1 = 3', o = k + 10 for k < 0 and k + 9 for k > 0.
Lengths: only records whose seg is neither 'f' nor 'b'; the others count in `halves`.  Length = the columns c in 0 .. n-1 with
seq[c] != '-' plus the characters other than '-' of the INS_POS pairs (pos, string) with 0 <= pos <= n-1 that no later pair of the
record repeats.  len_count[rc][min(length, 512)].
"""
import numpy as np

REACH, MAX_LEN = 10, 512
KS = tuple(range(-REACH, 0)) + tuple(range(1, REACH + 1))
_CLASS = {"A": 0, "a": 0, "C": 1, "c": 1, "G": 2, "g": 2, "T": 3, "t": 3}


def seg_of(r):
    return r["seg"][:1]


def counted(m, use_dropped=False):
    return [r for r in m.rec if use_dropped or not r["dr"]]


def anchors(r):
    """[(end, anchor column)] of the record's true ends: end 0 = 5', 1 = 3'"""
    s, e, seg = r["start"], r["end"], seg_of(r)
    out = []
    if r["rc"]:
        if seg != "f":
            out.append((0, e))
        if seg != "b":
            out.append((1, s))
    else:
        if seg != "b":
            out.append((0, s))
        if seg != "f":
            out.append((1, e))
    return out


def column(end, a, d, k):
    if end == 0:
        return a + d * (k - 1) if k > 0 else a + d * k
    return a + d * (k + 1) if k < 0 else a + d * k


def klass(L, ref_seq, p, rc):
    if p < 0 or p > L - 1:
        return 5
    c = _CLASS.get(ref_seq[p], 4)
    return 3 - c if rc and c < 4 else c


def slot(k):
    return k + 10 if k < 0 else k + 9


def length(r):
    n = r["end"] - r["start"] + 1
    total = sum(1 for c in range(n) if r["seq"][c] != "-")
    for j, (pos, text) in enumerate(r["ins"]):
        if 0 <= pos <= n - 1 and not any(later == pos for later, _ in r["ins"][j + 1:]):
            total += sum(1 for ch in text if ch != "-")
    return total


def counts_split(m):
    """[(ctx[2, 20, 6], len_count[2, 513], halves) of the records not marked DR, the same of those marked DR]"""
    out = [[np.zeros((2, 20, 6), np.int64), np.zeros((2, MAX_LEN + 1), np.int64), 0] for _ in range(2)]
    for r in m.rec:
        acc = out[1 if r["dr"] else 0]
        rc = 1 if r["rc"] else 0
        d = -1 if rc else 1
        for end, a in anchors(r):
            for k in KS:
                acc[0][end, slot(k), klass(m.L, m.ref_seq, column(end, a, d, k), rc)] += 1
        if seg_of(r) in ("f", "b"):
            acc[2] += 1
        else:
            acc[1][rc, min(length(r), MAX_LEN)] += 1
    return tuple(out[0]), tuple(out[1])


def counts(m, use_dropped=False, split=None):
    """(ctx, len_count, halves) of the records that count"""
    kept, dropped = counts_split(m) if split is None else split
    return (kept[0] + dropped[0], kept[1] + dropped[1], kept[2] + dropped[2]) if use_dropped else kept


def n_ends(ctx):
    """(5' ends, 3' ends): every end adds one event to each of its positions"""
    return int(ctx[0, 0].sum()), int(ctx[1, 0].sum())


def ends_table(m, use_dropped=False, cnt=None):
    """-f 92"""
    ctx = (counts(m, use_dropped) if cnt is None else cnt)[0]
    n5, n3 = n_ends(ctx)
    out = ["# ma_hip fragment ends: %d records, %d 5' ends, %d 3' ends\n" % (len(counted(m, use_dropped)), n5, n3),
           "# end\tposition\tA\tC\tG\tT\tother\toutside\n"]
    for end, label in ((0, "5p"), (1, "3p")):
        for k in KS:
            out.append("%s\t%+d" % (label, k) + "".join("\t%d" % x for x in ctx[end, slot(k)]) + "\n")
    return "".join(out)


def lengths_table(m, use_dropped=False, cnt=None):
    """-f 93"""
    _, lens, halves = counts(m, use_dropped) if cnt is None else cnt
    both = lens[0] + lens[1]
    out = ["# ma_hip read lengths: %d whole records, %d halves of reads split at the origin (not counted), %d longer than 511\n" %
           (int(both.sum()), halves, int(both[MAX_LEN])), "# length\tforward\treverse\n"]
    seen = np.nonzero(both[:MAX_LEN])[0]
    if seen.size:
        for l in range(int(seen[0]), int(seen[-1]) + 1):
            out.append("%d\t%d\t%d\n" % (l, lens[0, l], lens[1, l]))
    if both[MAX_LEN]:
        out.append(">511\t%d\t%d\n" % (lens[0, MAX_LEN], lens[1, MAX_LEN]))
    return "".join(out)


def true_ends(m):
    """{reference column: [forward starts, reverse starts, forward ends, reverse ends]} of every record, dropped or not, non-zero
    columns only: what columns 5-8 of the reference's `ma -f 3` print for that column.  A forward 5' end is a forward start, a
    forward 3' end a forward end, a reverse 3' end a reverse start, a reverse 5' end a reverse end."""
    out = {}
    for r in m.rec:
        for end, a in anchors(r):
            which = (1 if end == 1 else 3) if r["rc"] else (0 if end == 0 else 2)
            out.setdefault(a, [0, 0, 0, 0])[which] += 1
    return out
