"""The strand-split column table (ma_hip -f 42) restated in numpy over a maln_synth.Maln.  The rule is the project's own (DESIGN.md,
"Strand table (-f 42)") and is written here from its text, sharing nothing with csrc/ma_cols_body.h.  Two places tie it to what the
reference does produce (tests/test_ma_cols_cpu.py): words 12 .. 15 are columns 5-8 of its own `ma -f 3`, and words 0 .. 11, added over
the two strands, are the base counts of its `-f 41`.

A record: s = START, n its columns, e = s + n - 1, rc, seg = the SEG character.  A record marked DR is left out unless dropped records
are asked for.  Sixteen words per reference column p in 0 .. L-1:
  column events   c = 0 .. n-1, p = s + c: p >= L adds one to `beyond` and nothing else; otherwise one to word (6 if rc else 0) +
                  class(seq[c]), the class of the exact character: A C G T -> 0 .. 3, '-' -> 4, anything else (lower case too) -> 5
  end events      word 12: not rc and seg != 'b', on s      word 13: rc and seg != 'b', on s
                  word 14: not rc and seg != 'f', on e      word 15: rc and seg != 'f', on e
                  a column outside 0 .. L-1 adds one to `ends_outside` and nothing else
n_used = the records that count, n_events = the sum of words 0 .. 11 plus beyond.
"""
import numpy as np

WORDS = 16
NAMES = ("A+", "C+", "G+", "T+", "gap+", "other+", "A-", "C-", "G-", "T-", "gap-", "other-", "starts+", "starts-", "ends+", "ends-")
_CLASS = np.full(256, 5, np.int64)
for _i, _ch in enumerate(b"ACGT-"):
    _CLASS[_ch] = _i


def seg_of(r):
    return r["seg"][:1]


def counted(m, use_dropped=False):
    return [r for r in m.rec if use_dropped or not r["dr"]]


def table(L, recs):
    """(cols int64 [16, L], n_used, n_events, beyond, ends_outside) of the records given, all of which count"""
    cols = np.zeros((WORDS, L), np.int64)
    if not recs:
        return cols, 0, 0, 0, 0
    s = np.array([r["start"] for r in recs], np.int64)
    n = np.array([r["end"] - r["start"] + 1 for r in recs], np.int64)
    e = s + n - 1
    rc = np.array([1 if r["rc"] else 0 for r in recs], np.int64)
    seg = np.array([ord(seg_of(r) or "n") for r in recs], np.int64)
    # column events: every column of every record, flat
    first = np.cumsum(n) - n
    chars = np.frombuffer("".join(r["seq"][:k] for r, k in zip(recs, n.tolist())).encode("latin1"), np.uint8)
    assert len(chars) == int(n.sum())
    rec = np.repeat(np.arange(len(recs)), n)
    p = s[rec] + (np.arange(len(chars)) - first[rec])
    inside = p < L
    beyond = int((~inside).sum())
    word = 6 * rc[rec] + _CLASS[chars]
    cols[:12] = np.bincount(word[inside] * L + p[inside], minlength=12 * L).reshape(12, L)
    # end events
    outside = 0
    for base, there, a in ((12, seg != ord("b"), s), (14, seg != ord("f"), e)):
        for strand in (0, 1):
            mine = there & (rc == strand)
            on = mine & (a >= 0) & (a <= L - 1)
            cols[base + strand] = np.bincount(a[on], minlength=L)
            outside += int((mine & ~on).sum())
    return cols, len(recs), int(cols[:12].sum()) + beyond, beyond, outside


def counts(m, use_dropped=False):
    return table(m.L, counted(m, use_dropped))


def region(text, L):
    """-R a:b as ma reads it: 1-based inclusive; a > b makes both the smaller one; clamped to 1 .. L.  (first, last), 0-based inclusive;
    first > last: no rows"""
    a, b = (int(x) for x in text.split(":"))
    if a > b:
        a = b
    return max(a, 1) - 1, min(b, L) - 1


def report(m, use_dropped=False, cnt=None, rows=None):
    """-f 42; rows: (first, last) of region(), None: every column"""
    cols, n_used, n_events, beyond, outside = counts(m, use_dropped) if cnt is None else cnt
    first, last = (0, m.L - 1) if rows is None else rows
    out = ["# ma_hip strand table: %d records, %d columns, %d beyond the reference, %d ends outside it\n" % (n_used, n_events, beyond, outside),
           "# position\treference\t" + "\t".join(NAMES) + "\n"]
    for p in range(first, last + 1):
        out.append("%d\t%s\t" % (p + 1, m.ref_seq[p]) + "\t".join("%d" % x for x in cols[:, p]) + "\n")
    return "".join(out)
