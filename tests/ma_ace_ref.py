"""ace_output (reference src/io.c:756-913) and write_ma (src/map_alignment.c:283-382) restated in Python over a maln_synth.Maln,
as `ma` reaches them: records sorted by START, then END (equal ones keep their order), -c and -I applied.  tests/test_ma_ace_cpu.py
holds both against the recorded output of the reference itself, so that a GPU test can name the record and the character that differ.
"""
import copy

import numpy as np

import maln_synth as ms

INIT_NUM_ALN_SEQS = 16000                  # src/params.h:69
LINE = 50


def sorted_records(m):
    return sorted(m.rec, key=lambda r: (r["start"], r["end"]))


def ins_table(r):
    """aln_seq->ins[]: of several pairs of one position the last one read stays (src/map_alignment.c:602-605)"""
    t = {}
    for p, s in r["ins"]:
        t[p] = s
    return t


def consensus(m, cons_code):
    """get_consensus (src/map_alignment.c:229-278): every column's call, in front of every column but the first its insert columns'
    calls, '-' kept.  The tallies are maln_synth's; pairs the reference never looks at (position 0, behind END, replaced) are left out."""
    m2 = copy.copy(m)
    m2.rec = []
    for r in m.rec:
        r2 = dict(r)
        r2["end"] = min(r["end"], m.L - 1)         # (a circular assembly's record may end on column L: no column of the consensus)
        ncols = r2["end"] - r["start"] + 1
        r2["ins"] = sorted((p, s) for p, s in ins_table(r).items() if 0 < p < ncols)
        m2.rec.append(r2)
    rs = ms.restate(m2)
    cc, ic = rs.calls(cons_code)
    out = []
    for p in range(m.L):
        if p > 0 and m.gaps[p] > 0:
            out.append(ic[int(rs.ins_off[p]):int(rs.ins_off[p]) + int(m.gaps[p])])
        out.append(cc[p])
    return "".join(out)


def lines50(s):
    """lines of 50 and the remainder line, which is there even when it is empty"""
    full = len(s) // LINE * LINE
    return "".join(s[i:i + LINE] + "\n" for i in range(0, full, LINE)) + s[full:] + "\n"


def layout(m):
    """per sorted record: (af_pos, padded_len, padded read) -- padded_len is the length of the padded read, without what SEQ holds behind END"""
    G = np.concatenate(([0], np.cumsum(m.gaps.astype(np.int64))))
    G = np.append(G, G[-1])                        # ace_output sets gaps[L] = 0: a record may end on column L
    gaps = np.append(m.gaps, 0)
    out = []
    for r in sorted_records(m):
        s, e = r["start"], r["end"]
        ins = ins_table(r)
        chars = []
        for i in range(s, e + 1):
            g = int(gaps[i])
            if g > 0:
                have = ins.get(i - s, "")[:g]
                chars.append(have + "*" * (g - len(have)))
            chars.append(r["seq"][i - s])
        text = "".join(chars).replace("-", "*")
        assert len(text) == (e - s + 1) + int(G[e + 1] - G[s])
        out.append((s + int(G[s]) + 1, len(text), text))
    return out


def ace(m, cons_code=1, assign_id=None):
    assert m.gaps[0] <= 0 and (m.gaps >= 0).all(), "no ACE export: the reference reads past its consensus string"
    cons = consensus(m, cons_code)
    nb = m.L + int(m.gaps.sum())
    assert len(cons) == nb
    recs = sorted_records(m)
    shown = lines50(cons.replace("-", "*").replace(" ", "X"))
    out = ["AS 1 %d\n\n" % (len(recs) + 1), "CO %s %d %d 1 U\n" % (assign_id if assign_id is not None else m.ref_id, nb, len(recs) + 1), shown, "\nBQ\n"]
    for i, c in enumerate(cons):
        if c != "-":
            out.append("40 ")
        if i % LINE == 0:
            out.append("\n")
    out.append("\n\nAF FAKE_READ-IGNORE_ME U 1\n")
    lay = layout(m)
    for r, (af, _, _) in zip(recs, lay):
        out.append("AF %s %s %d\n" % (r["id"], "C" if r["rc"] else "U", af))
    out.append("\nBS 1 %d FAKE_READ-IGNORE_ME\n\n" % len(cons))
    for r, (_, plen, text) in zip(recs, lay):
        n = plen + len(r["seq"]) - (r["end"] - r["start"] + 1)
        out.append("RD %s %d 0 0\n%s\nQA 1 %d 1 %d\nDS CHROMAT_FILE: %s PHD_FILE: %s_FAKE.phd TIME: Tue Feb 21 15:42:35 1984\n\n" %
                   (r["id"], n, lines50(text), n, n, r["id"], r["id"]))
    out.append("RD FAKE_READ-IGNORE_ME %d 0 0\n%s\n\nQA 1 %d 1 %d\n" % (nb, shown, nb, nb))
    out.append("DS CHROMAT_FILE: FAKE_READ PHD_FILE: FAKE_READ_FAKE.phd TIME: Tue Feb 21 23:23:23 1984\n")
    return "".join(out)


def rewrite(m, cons_code=1, assign_id=None):
    """what `ma -m` writes, from the MALN_NAS line on"""
    w = copy.copy(m)
    w.siz = INIT_NUM_ALN_SEQS
    while w.siz < m.siz:                   # read_ma doubles its record array until it is as large as MALN_SIZ says
        w.siz *= 2
    w.coc = cons_code
    if assign_id is not None:
        w.ref_id = assign_id
    w.ref_desc = (m.ref_desc.split() or [""])[0]
    w.rec = []
    for r in sorted_records(m):
        r2 = dict(r)
        r2["num_inputs"] = 1 if r["num_inputs"] is None else r["num_inputs"]
        r2["dr"] = 1 if r["dr"] else 0
        r2["rc"], r2["tr"] = (1 if r["rc"] else 0), (1 if r["tr"] else 0)
        r2["seg"] = r["seg"][:1]
        r2["ins"] = sorted((p, s) for p, s in ins_table(r).items() if 0 <= p < len(r["seq"]))
        w.rec.append(r2)
    return ms.write_maln(w)


def expected(m, key, args):
    """(stdout or None when this module does not restate it, file text from line 2 on or None) of a run of maln_ace_cases.RUNS"""
    code = int(args[args.index("-c") + 1]) if "-c" in args else 1
    new_id = args[args.index("-I") + 1] if "-I" in args else None
    fmt = int(args[args.index("-f") + 1]) if "-f" in args else 1
    out = ace(m, code, new_id) if fmt == 7 else None
    return out, (rewrite(m, code, new_id) if "-m" in args else None)
