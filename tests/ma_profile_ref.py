"""The substitution profile of ma_hip (-f 9, -f 91) restated in Python over a maln_synth.Maln.  The reference's `ma` has no such
report, so nothing recorded from it can pin this one; the rule below is the project's own ("Substitution profile") and is
written here from its text, not from csrc/ma_profile_body.h.

A record covers columns START .. END, n = END - START + 1, of a reference of L characters.  A record marked DR is left out unless
dropped records are asked for.  For a record that counts and c = 0 .. n-1, p = START + c:
  1. p >= L: the column counts in `beyond` and nowhere else;
  2. else d = SMP[c] - 'A' outside 0 .. 30: it counts in `bad_code` and nowhere else;
  3. else i = class of upper(ref_seq[p]), j = class of upper(SEQ[c]) (A C G T -> 0 1 2 3, anything else 4).  A record with RC set is
     stored reverse-complemented: d' = 30 - d, i' = 3 - i if i < 4 else 4, j' likewise; otherwise d' = d, i' = i, j' = j;
  4. SEQ[c] == '-': del[d'] += 1 (i is not looked at), else count[d'][i'][j'] += 1.
INS_POS pairs are not looked at; NUM_INPUTS does not weigh.
"""
import math

import numpy as np

LABELS = [str(d + 1) for d in range(15)] + ["MIDDLE"] + [str(d - 31) for d in range(16, 31)]
MIN_ALPHA, MAX_ALPHA = 1e-60, 1e60
N_SCORE, NR_SCORE = -100, -10              # src/params.h:30-31


_CLASS = {"A": 0, "a": 0, "C": 1, "c": 1, "G": 2, "g": 2, "T": 3, "t": 3}       # upper(ch) in A C G T; anything else is class 4


def _class(ch):
    return _CLASS.get(ch, 4)


def event(L, ref_seq, start, c, seq_ch, smp_ch, rc):
    """where one column counts: ("beyond",), ("bad_code",), ("del", d') or ("count", d', i', j')"""
    p = start + c
    if p >= L:
        return ("beyond",)
    d = ord(smp_ch) - ord("A")
    if d < 0 or d > 30:
        return ("bad_code",)
    i, j = _class(ref_seq[p]), _class(seq_ch)
    if rc:
        d, i, j = 30 - d, (3 - i if i < 4 else 4), (3 - j if j < 4 else 4)
    if seq_ch == "-":
        return ("del", d)
    return ("count", d, i, j)


def counted(m, use_dropped=False):
    """the records that count"""
    return [r for r in m.rec if use_dropped or not r["dr"]]


def profile_split(m):
    """((count[31, 5, 5], del[31], bad_code, beyond) of the records not marked DR, the same of those marked DR): a plain loop over
    records and columns"""
    out = [[np.zeros((31, 5, 5), np.int64), np.zeros(31, np.int64), 0, 0] for _ in range(2)]
    for r in m.rec:
        count, dele = out[1 if r["dr"] else 0][:2]
        bad = beyond = 0
        for c in range(r["end"] - r["start"] + 1):
            e = event(m.L, m.ref_seq, r["start"], c, r["seq"][c], r["smp"][c], bool(r["rc"]))
            if e[0] == "beyond":
                beyond += 1
            elif e[0] == "bad_code":
                bad += 1
            elif e[0] == "del":
                dele[e[1]] += 1
            else:
                count[e[1], e[2], e[3]] += 1
        out[1 if r["dr"] else 0][2] += bad
        out[1 if r["dr"] else 0][3] += beyond
    return tuple(out[0]), tuple(out[1])


def profile(m, use_dropped=False, split=None):
    """(count[31, 5, 5], del[31], bad_code, beyond) of the records that count"""
    kept, dropped = profile_split(m) if split is None else split
    return (kept[0] + dropped[0], kept[1] + dropped[1], kept[2] + dropped[2], kept[3] + dropped[3]) if use_dropped else kept


def table(m, use_dropped=False, prof=None):
    """-f 9"""
    count, dele, bad, beyond = profile(m, use_dropped) if prof is None else prof
    events = int(count.sum() + dele.sum()) + bad + beyond
    out = ["# ma_hip substitution profile: %d records, %d columns, %d bad depth codes, %d columns beyond the reference\n" %
           (len(counted(m, use_dropped)), events, bad, beyond),
           "# position" + "".join("\t%s>%s" % (a, b) for a in "ACGT" for b in "ACGT") + "\tdel\tother\n"]
    for d in range(31):
        other = int(count[d].sum() - count[d, :4, :4].sum())
        out.append(LABELS[d] + "".join("\t%d" % count[d, i, j] for i in range(4) for j in range(4)) + "\t%d\t%d\n" % (dele[d], other))
    return "".join(out)


def score(row, i, j, alpha):
    """the entry of ref class i, read class j from the four counts of ref class i"""
    n = int(sum(int(x) for x in row))
    if n == 0:
        return 200 if i == j else -600
    return math.floor(100.0 * math.log2(((float(int(row[j])) + alpha) / (float(n) + 4.0 * alpha)) / 0.25) + 0.5)


def scores(count, alpha):
    """[31][4][4]"""
    return [[[score(count[d, i, :4], i, j, alpha) for j in range(4)] for i in range(4)] for d in range(31)]


def matrix(m, alpha=1.0, use_dropped=False, prof=None):
    """-f 91"""
    if not (math.isfinite(alpha) and MIN_ALPHA <= alpha <= MAX_ALPHA):
        raise ValueError("pseudocount")
    count = (profile(m, use_dropped) if prof is None else prof)[0]
    sc = scores(count, alpha)
    return "".join("# Matrix for position: %s\n" % LABELS[d] + "".join("%d\t%d\t%d\t%d\t\n" % tuple(sc[d][i]) for i in range(4)) + "\n" for d in range(31))


def read_pssm(text):
    """read_pssm (src/io.c:408-503) over the text of a matrix file: 31 blocks of a title line, four lines read with
    "%d\\t%d\\t%d\\t%d" and a line that is skipped; block 15 must say MIDDLE.  sm[31][5][5]: column 4 of rows 0 .. 3 is N_SCORE, row 4
    is NR_SCORE (:443-448)."""
    lines = text.split("\n")
    sm = np.zeros((31, 5, 5), np.int64)
    k = 0
    for d in range(31):
        title = lines[k]
        k += 1
        assert ("# Matrix for position: MIDDLE" if d == 15 else "# Matrix for position") in title, (d, title)
        for base in range(4):
            f = lines[k].split("\t")
            k += 1
            sm[d, base, :4] = [int(f[0]), int(f[1]), int(f[2]), int(f[3])]
            sm[d, base, 4] = N_SCORE
        sm[d, 4, :] = NR_SCORE
        k += 1                             # the blank line
    return sm
