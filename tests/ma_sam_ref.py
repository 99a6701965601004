"""The SAM export of ma_hip (-f 8) restated in Python over a maln_synth.Maln.  The reference's `ma` has no SAM output, so nothing
recorded from it can pin this report; the rule below is the project's own ("SAM export") and is written here from its
text, not from csrc/ma_sam_body.h.  `rebuild` is the way back: from a SAM line to the record's columns, inserts and marks.

A record covers columns START .. END, n = END - START + 1, on a reference of L columns.  Walk c = 0 .. n-1:
  1. the insert the record has at position c comes first (of several INS_POS pairs of one position the last one given; pairs of a
     position outside 0 .. n-1 are never looked at): its characters other than '-' go to SEQ, whole, each as op I -- op S when
     START + c >= L;
  2. then the column's own character: '-' is op D and no SEQ character (nothing at all when START + c >= L); any other character
     goes to SEQ as it stands, as op M -- op S when START + c >= L;
  3. equal neighbouring ops merge; a run prints as its decimal length and its letter.
A record without columns, or whose walk yields no SEQ character, prints CIGAR * and SEQ *.
NM = the D ops + the I ops + the M columns whose character differs from ref_seq[START + c], both upper-cased (N against a base is
a difference); soft-clipped characters do not count.
"""
import itertools
import re

MID = "\t*\t0\t0\t"


def sorted_records(m):
    """ma's order (sort_records: stable, by START then END)"""
    return sorted(m.rec, key=lambda r: (r["start"], r["end"]))


def ins_table(r):
    t = {}
    for p, s in r["ins"]:
        t[p] = s
    return t


def _up(ch):
    return ch.upper() if "a" <= ch <= "z" else ch


def walk(r, L, ref_seq):
    """(ops, seq, nm): one op letter per op, the SEQ characters, NM"""
    s, n = r["start"], r["end"] - r["start"] + 1
    ins = ins_table(r)
    ops, seq, nm = [], [], 0
    for c in range(n):
        clip = s + c >= L
        for ch in ins.get(c, ""):
            if ch != "-":
                seq.append(ch)
                ops.append("S" if clip else "I")
                nm += 0 if clip else 1
        ch = r["seq"][c]
        if ch == "-":
            if not clip:
                ops.append("D")
                nm += 1
        else:
            seq.append(ch)
            if clip:
                ops.append("S")
            else:
                ops.append("M")
                nm += 1 if _up(ch) != _up(ref_seq[s + c]) else 0
    return "".join(ops), "".join(seq), nm


def fields(r, L, ref_seq):
    """(CIGAR, SEQ, NM) as printed"""
    ops, seq, nm = walk(r, L, ref_seq)
    if not seq:
        return "*", "*", nm
    return "".join("%d%s" % (len(list(g)), k) for k, g in itertools.groupby(ops)), seq, nm


def body(r, L, ref_seq):
    """(fields 6-10 of the record's line, NM)"""
    cigar, seq, nm = fields(r, L, ref_seq)
    return cigar + MID + seq, nm


def flag(r):
    return (16 if r["rc"] else 0) + (512 if r["dr"] else 0) + (2048 if r["seg"][:1] == "b" else 0)


def header(ref_id, L):
    return "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:%s\tLN:%d\n@PG\tID:ma_hip\tPN:ma_hip\n" % (ref_id, L)


def line(r, ref_id, L, ref_seq):
    b, nm = body(r, L, ref_seq)
    return "%s\t%d\t%s\t%d\t255\t%s\t*\tAS:i:%d\tNM:i:%d\tXN:i:%d\tXS:A:%s\tXT:i:%d\n" % (
        r["id"], flag(r), ref_id, r["start"] + 1, b, r["score"], nm, 1 if r["num_inputs"] is None else r["num_inputs"], r["seg"][:1], 1 if r["tr"] else 0)


def sam(m, assign_id=None):
    """what ma_hip -f 8 [-I assign_id] prints"""
    rid = m.ref_id if assign_id is None else assign_id
    return header(rid, m.L) + "".join(line(r, rid, m.L, m.ref_seq) for r in sorted_records(m))


def cigar_runs(cigar):
    """[(length, letter)]; [] for *"""
    if cigar == "*":
        return []
    runs = re.findall(r"(\d+)([MIDS])", cigar)
    assert "".join(a + b for a, b in runs) == cigar, cigar
    return [(int(a), b) for a, b in runs]


def query_len(cigar):
    return sum(k for k, op in cigar_runs(cigar) if op in "MIS")


def ref_len(cigar):
    return sum(k for k, op in cigar_runs(cigar) if op in "MD")


def rebuild(sam_line, ref_seq):
    """From a SAM line back to the record: its column string below the reference's end ('-' where the CIGAR deletes; None when
    the CIGAR is *, which keeps no count of columns), its (position, insert) list below the reference's end (inserts without their
    '-'; an insert of nothing but '-' leaves no trace), the soft-clipped characters, and what FLAG, POS and the tags say.
    ref_seq serves NM: the direct count over the rebuilt columns is returned beside the line's own."""
    f = sam_line.rstrip("\n").split("\t")
    assert len(f) == 16 and f[4] == "255" and f[6:9] == ["*", "0", "0"] and f[10] == "*", f[:11]
    fl, start, cigar, seq = int(f[1]), int(f[3]) - 1, f[5], f[9]
    tags = dict((t[:4], t[5:]) for t in f[11:])
    out = {"id": f[0], "rname": f[2], "start": start, "rc": 1 if fl & 16 else 0, "dr": 1 if fl & 512 else 0, "seg_b": bool(fl & 2048),
           "flag_rest": fl & ~(16 | 512 | 2048), "score": int(tags["AS:i"]), "nm": int(tags["NM:i"]), "num_inputs": int(tags["XN:i"]),
           "seg": tags["XS:A"], "tr": int(tags["XT:i"])}
    if cigar == "*":
        assert seq == "*"
        out.update(columns=None, ins=[], clipped="", nm_count=None)
        return out
    cols, ins, clipped, at, nm = [], [], [], 0, 0
    for k, op in cigar_runs(cigar):
        if op == "M":
            for ch in seq[at:at + k]:
                nm += 1 if _up(ch) != _up(ref_seq[start + len(cols)]) else 0
                cols.append(ch)
        elif op == "D":
            cols.extend("-" * k)
            nm += k
        elif op == "I":
            ins.append((len(cols), seq[at:at + k]))
            nm += k
        else:
            clipped.append(seq[at:at + k])
        at += k if op != "D" else 0
    assert at == len(seq)
    out.update(columns="".join(cols), ins=ins, clipped="".join(clipped), nm_count=nm)
    return out


def expected_rebuild(r, L):
    """what rebuild must give for record r: (columns below L, inserts below L without '-', clipped characters)"""
    s, n = r["start"], r["end"] - r["start"] + 1
    below = max(0, min(n, L - s))
    t = ins_table(r)
    ins = [(c, t[c].replace("-", "")) for c in sorted(t) if 0 <= c < below and t[c].replace("-", "")]
    clipped = "".join(t.get(c, "").replace("-", "") + r["seq"][c].replace("-", "") for c in range(below, n))
    return r["seq"][:below], ins, clipped
