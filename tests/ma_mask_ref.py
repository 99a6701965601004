"""The end mask of ma_hip (-E, -x, -f 96) restated in Python over a maln_synth.Maln, from the text of DESIGN.md ("End mask"): a loop over
records and columns.  Nothing here is shared with the kernels or with csrc/ma_mask_body.h.

  column c of a record: d = smp[c] - 'A'; d' = d (forward) or 30 - d (RC)
  5' zone: d in 0 .. 30 and d' < n5, position k = d' + 1;   3' zone: d in 0 .. 30 and d' > 30 - n3, position k = 31 - d'
  trim: a = leading zone columns, b = n - trailing zone columns (not below a), then a forward and b backward over '-'; a >= b: emptied
  -x:   a 5' zone column whose base in the read's orientation is T, a 3' zone column whose base is A (-S: T), becomes N
"""
import copy

import numpy as np

import ma_dedup_ref

SETTINGS = ((3, 3, False, False), (10, 10, False, False), (15, 15, False, False), (5, 0, False, False), (0, 2, False, False),
            (3, 3, True, False), (15, 15, True, False), (3, 3, True, True))
COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A"}


def tag(n5, n3, substitute, ss):
    return "%d_%d_%s" % (n5, n3, "trim" if not substitute else "Nss" if ss else "N")


def zones(smp_ch, rc, n5, n3):
    """(k at the 5' end or 0, k at the 3' end or 0) of a column"""
    d = ord(smp_ch) - ord("A")
    if not 0 <= d <= 30:
        return 0, 0
    dd = 30 - d if rc else d
    return (dd + 1 if dd < n5 else 0), (31 - dd if dd > 30 - n3 else 0)


def read_base(seq_ch, rc):
    """the column's base in the read's orientation, upper-cased; None for what is no base"""
    b = seq_ch.upper()
    if b not in COMPLEMENT:
        return None
    return COMPLEMENT[b] if rc else b


class Masked:
    """the masked Maln and everything mia_hip_get_ma_mask hands out, in the record and pair order of maln_synth.flatten"""

    def __init__(self, n):
        self.maln = None
        self.first, self.count, self.start = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
        self.col_off = np.zeros(n + 1, np.int64)
        self.seq, self.smp = b"", b""
        self.pair_keep, self.ins_pos = [], []
        self.hist = np.zeros((2, 2, 16), np.int64)
        self.emptied = [0, 0]
        self.stripped = self.pairs_dropped = self.n_kept = self.cols_kept = 0

    def counts(self):
        return {"hist": self.hist.reshape(-1).tolist(), "emptied": list(self.emptied), "stripped": self.stripped, "pairs_dropped": self.pairs_dropped,
                "n_kept": self.n_kept, "cols_kept": self.cols_kept}


def mask(m, n5, n3, substitute=False, ss=False):
    assert 0 <= n5 <= 15 and 0 <= n3 <= 15 and (n5 or n3) and (substitute or not ss)
    out = Masked(len(m.rec))
    recs, seqs, smps = [], [], []
    by_code = [[zones(chr(x), rc, n5, n3) for x in range(256)] for rc in (0, 1)]          # (looked up per column: the files are large)
    for r, rec in enumerate(m.rec):
        rc = 1 if rec["rc"] else 0
        n = rec["end"] - rec["start"] + 1
        seq, smp = rec["seq"][:n], rec["smp"][:n]
        z = [by_code[rc][x] for x in smp.encode("latin1")]
        out.start[r] = rec["start"]
        if substitute:
            new = list(seq)
            for c in range(n):
                if z[c] == (0, 0):
                    continue
                base = read_base(seq[c], rc)
                if z[c][0] and base == "T":
                    new[c] = "N"
                    out.hist[rc, 0, z[c][0]] += 1
                elif z[c][1] and base == ("T" if ss else "A"):
                    new[c] = "N"
                    out.hist[rc, 1, z[c][1]] += 1
            new = "".join(new)
            out.first[r], out.count[r] = 0, n
            out.pair_keep += [1] * len(rec["ins"])
            out.ins_pos += [p for p, _ in rec["ins"]]
            recs.append(dict(rec, seq=new + rec["seq"][n:]))
            seqs.append(new)
            smps.append(smp)
            continue
        a = 0
        while a < n and (z[a][0] or z[a][1]):
            a += 1
        b = n
        while b > a and (z[b - 1][0] or z[b - 1][1]):
            b -= 1
        while a < b and seq[a] == "-":
            a += 1
        while b > a and seq[b - 1] == "-":
            b -= 1
        for c in (range(n) if a >= b else list(range(a)) + list(range(b, n))):       # the columns that leave
            if z[c][0]:
                out.hist[rc, 0, z[c][0]] += 1
            elif z[c][1]:
                out.hist[rc, 1, z[c][1]] += 1
            else:
                out.stripped += 1
        if a >= b:
            out.emptied[rc] += 1
            out.pair_keep += [0] * len(rec["ins"])
            out.ins_pos += [0] * len(rec["ins"])
            continue
        out.first[r], out.count[r], out.start[r] = a, b - a, rec["start"] + a
        ins = []
        for p, s in rec["ins"]:
            if a < p < b:
                ins.append((p - a, s))
                out.pair_keep.append(1)
                out.ins_pos.append(p - a)
            else:
                out.pairs_dropped += 1
                out.pair_keep.append(0)
                out.ins_pos.append(0)
        recs.append(dict(rec, start=rec["start"] + a, end=rec["start"] + b - 1, seq=seq[a:b], smp=smp[a:b], ins=ins))
        seqs.append(seq[a:b])
        smps.append(smp[a:b])
    np.cumsum(out.count, out=out.col_off[1:])
    out.seq, out.smp = "".join(seqs).encode("latin1"), "".join(smps).encode("latin1")
    out.pair_keep, out.ins_pos = np.array(out.pair_keep, np.uint8), np.array(out.ins_pos, np.int32)
    out.n_kept, out.cols_kept = len(recs), int(out.col_off[-1])
    out.maln = copy.copy(m)
    out.maln.rec = recs
    if not substitute:
        out.maln.gaps = ma_dedup_ref.new_gaps(out.maln, [1] * len(recs))
    return out


def report_of(n_in, counts, substitute, ss):
    """-f 96 from the counts alone"""
    hist = np.array(counts["hist"], np.int64).reshape(2, 2, 16)
    out = ["# ma_hip end mask: %d records, %d kept, %d %d emptied, %d inserts dropped, %d gap columns stripped, mode %s, library %s\n" %
           (n_in, counts["n_kept"], counts["emptied"][0], counts["emptied"][1], counts["pairs_dropped"], counts["stripped"], "N" if substitute else "trim",
            "ss" if ss else "ds"), "# k\t5p+\t5p-\t3p+\t3p-\n"]
    for k in range(1, 16):
        out.append("%d\t%d\t%d\t%d\t%d\n" % (k, hist[0, 0, k], hist[1, 0, k], hist[0, 1, k], hist[1, 1, k]))
    return "".join(out)


def report(m, n5, n3, substitute=False, ss=False):
    return report_of(len(m.rec), mask(m, n5, n3, substitute, ss).counts(), substitute, ss)
