"""The .maln files of the ACE export (ma -f 7) and of the rewrite (ma -m): the smallest shapes at which each piece can go wrong.

  CASES / make_case   every case as a maln_synth.Maln, rebuilt from fixed seeds (the texts are never committed):
                        shapes      hand-placed records: padded lengths 1, 49, 50, 51, 99, 100, 101 and a few hundred; both strands;
                                    segments a, f, b, n; a record at column 0 and one ending at L - 1; '-' in SEQ and in an insert;
                                    records whose first column has insert columns, with and without an insert at position 0 (and
                                    two pairs for position 0: the later one counts); inserts shorter than, equal to and longer than
                                    GAPS; a SEQ longer than END - START + 1 (with an insert behind END); two pairs of records that
                                    compare equal; a record with dozens of INS_POS pairs given out of order; a record without columns
                        column300   2 000 records over one insert column of 300
                        empty       no records
                        the cases of maln_synth (edge255/256/257, scan16_4095/4096/4097, codes_anc, codes_flat) with GAPS[0] = 0:
                                    maln_synth sets GAPS[0] = 3, which has no ACE export
                        fix_c.1, fix_c.2, fix_lin.1 of tests/golden/maln
  REFUSED             gaps0: GAPS[0] > 0, for the refusal only
  SCAN_EDGES / make_records   recs_1023, recs_1024, recs_1025, recs_2049: that many short records -- one record less than, exactly and one
                      more than the 1 024 a workgroup of k_ma_region_select and k_ma_ace_layout takes, and two such workgroups and one
                      record (128 workgroups of k_ma_sam_layout less one record, 128, 128 and one record, 256 and one record).  They
                      are held to the restatements only: no run of the reference is recorded for them, so they are not in CASES
  RUNS                the recorded runs: arguments behind `-M <file>`; "OUT" stands for the path -m writes
"""
import copy
import os

import numpy as np

import maln_synth as ms

SYNTH = ("edge255", "edge256", "edge257", "scan16_4095", "scan16_4096", "scan16_4097", "codes_anc", "codes_flat")
FIXTURES = ("fix_c.1", "fix_c.2", "fix_lin.1")
CASES = ("shapes", "column300", "empty") + SYNTH + FIXTURES
REFUSED = ("gaps0",)
SCAN_EDGES = ("recs_1023", "recs_1024", "recs_1025", "recs_2049")
RECS_L, RECS_HOT = 300, {60: 2, 150: 3, 240: 1}           # make_records: reference columns; the columns that have insert columns
RUNS = {
    "f7c1": ["-f", "7", "-c", "1"],
    "f7c2": ["-f", "7", "-c", "2"],
    "f7I": ["-f", "7", "-I", "my_contig"],
    "m": ["-m", "OUT"],                                     # the default report (-f 1) on stdout, the file beside it
    "mc2I": ["-c", "2", "-I", "my_contig", "-f", "5", "-m", "OUT"],
}
ACGT = np.frombuffer(b"ACGT", np.uint8)


def _smp(n):
    off = np.arange(n)
    back = n - 1 - off
    d = np.where(off < ms.PSSM_DEPTH, off, np.where(back < ms.PSSM_DEPTH, 2 * ms.PSSM_DEPTH - back, ms.PSSM_DEPTH))
    return (d + ord("A")).astype(np.uint8).tobytes().decode()


def _blank(name, L, rng, gaps):
    m = ms.Maln()
    m.siz, m.coc, m.ref_id, m.ref_desc, m.L, m.size = 16000, 1, name, "", L, 2 * L + 2
    m.ref_seq = ACGT[rng.integers(0, 4, L)].tobytes().decode()
    m.gaps = np.zeros(L, np.int32)
    for p, g in gaps.items():
        m.gaps[p] = g
    m.fpsm = ms.flat_pssm()
    m.rpsm = ms.revcom_pssm(m.fpsm)
    return m


def _record(m, rng, rid, start, ncols, rc=0, seg="n", ins=(), extra=0, dash=0.03, **kw):
    """a record over columns start .. start + ncols - 1: the reference with a few other bases and '-'; `extra` characters of SEQ
    and SMP behind END"""
    n = ncols + extra
    ref = np.frombuffer((m.ref_seq + "ACGT" * (extra // 4 + 1))[start:start + n].encode(), np.uint8)
    u = rng.random(n)
    seq = np.where(u < 0.04, ACGT[rng.integers(0, 4, n)], ref)
    seq = np.where((u >= 0.04) & (u < 0.04 + dash), ord("-"), seq).astype(np.uint8).tobytes().decode()
    r = {"id": rid, "desc": kw.get("desc", ""), "score": kw.get("score", 1000 + 13 * len(m.rec)), "num_inputs": kw.get("num_inputs", 1), "start": start,
         "end": start + ncols - 1, "rc": rc, "tr": kw.get("tr", 0), "dr": kw.get("dr", 0), "seg": seg, "seq": seq, "smp": _smp(n), "ins": list(ins)}
    m.rec.append(r)
    return r


def _bases(rng, k):
    return ACGT[rng.integers(0, 4, k)].tobytes().decode()


def make_shapes():
    rng = ms.Rng(7001)
    L = 600
    m = _blank("shapes", L, rng, {10: 2, 100: 3, 200: 1, 300: 150, 599: 2})
    # file order is not sorted order: the reference sorts by START, then END, and keeps the order of equal records
    _record(m, rng, "end_at_last", 560, 40, rc=1, seg="a", ins=[(39, "G")])                    # padded 42; ends at L - 1, insert shorter than GAPS there
    _record(m, rng, "len406", 280, 256, seg="f")                                                # 256 + 150, no insert: 150 '*'
    _record(m, rng, "len270", 250, 120, rc=1, seg="b", ins=[(50, _bases(rng, 150))])            # insert as long as GAPS
    _record(m, rng, "len249", 271, 99, ins=[(29, _bases(rng, 70))], tr=1)                       # 70 bases, 80 '*'
    _record(m, rng, "twin_b", 20, 50, rc=1, seg="a", dr=1)                                      # padded 50; equal to twin_a below: twin_b stays first
    _record(m, rng, "len1", 0, 1, seg="n", dash=0.0)                                            # padded 1, at column 0
    _record(m, rng, "len49", 20, 49, seg="f")
    _record(m, rng, "twin_a", 20, 50, seg="b")
    _record(m, rng, "len51", 21, 51, rc=1)
    _record(m, rng, "len99", 95, 96, seg="a", ins=[(5, "AC")])                                  # shorter than GAPS[100] = 3
    _record(m, rng, "len100", 96, 97, rc=1, seg="f", ins=[(4, "TGA")])                          # equal
    _record(m, rng, "len101", 97, 98, seg="b", ins=[(3, "CATGC")])                              # longer: cut off at 3
    _record(m, rng, "first_gap_none", 100, 60, rc=1)                                            # GAPS[START] = 3 and no insert there: three '*'
    _record(m, rng, "first_gap_ins", 100, 61, seg="a", ins=[(0, "GG"), (0, "A-"), (40, "T")])   # two pairs for position 0: "A-" counts, printed "A*"
    _record(m, rng, "first_gap_long", 100, 61, seg="f", ins=[(0, "AC-TT")])                     # equal to first_gap_ins; longer than GAPS
    _record(m, rng, "long_seq", 400, 30, rc=1, extra=5, ins=[(32, "ACG"), (7, "T")], num_inputs=3)   # SEQ of 35 for 30 columns; a pair behind END
    many = [(p, _bases(rng, 1 + p % 3)) for p in range(199, 0, -7)] + [(5, "TT"), (95, "ACG"), (195, "C"), (60, "A"), (60, "CC")]
    _record(m, rng, "many_ins", 5, 200, seg="b", ins=many, desc="a record with many pairs")     # 29 pairs in descending order, then five more
    _record(m, rng, "no_columns", 450, 0, dash=0.0)                                             # END = START - 1: an empty padded read
    _record(m, rng, "dashes", 120, 70, rc=1, dash=0.4)
    return m


def make_column300():
    rng = ms.Rng(7002)
    L, n, col, g = 400, 2000, 200, 300
    m = _blank("column300", L, rng, {col: g})
    length = rng.integers(50, 151, n)
    back = rng.integers(1, 50, n)                          # the column is position `back` of the record
    ilen = np.where(rng.random(n) < 0.2, 0, rng.integers(1, g + 1, n))
    for i in range(n):
        ins = [(int(back[i]), _bases(rng, int(ilen[i])))] if ilen[i] else []
        _record(m, rng, "r%d" % i, col - int(back[i]), int(length[i]), rc=i & 1, seg="afbn"[i % 4], ins=ins)
    m.rec[0]["ins"] = [(int(back[0]), _bases(rng, g))]     # one insert of the full width
    return m


def make_records(n):
    """n records of 20 .. 40 columns on RECS_L reference columns, GAPS[0] = 0; every fifth has one INS_POS pair, behind its first
    column and in front of one of the RECS_HOT columns, of 1 .. GAPS bases"""
    rng = ms.Rng(7100 + n)
    m = _blank("recs_%d" % n, RECS_L, rng, RECS_HOT)
    hot = sorted(RECS_HOT)
    length = rng.integers(20, 41, n)
    start = rng.integers(0, RECS_L - 40, n)
    pos = rng.integers(1, 20, n)
    which = rng.integers(0, len(hot), n)
    for i in range(n):
        if i % 5 == 0:
            h = hot[int(which[i])]
            ins = [(int(pos[i]), _bases(rng, 1 + i // 5 % RECS_HOT[h]))]
            _record(m, rng, "s%d" % i, h - int(pos[i]), int(length[i]), rc=i & 1, seg="afbn"[i % 4], ins=ins)
        else:
            _record(m, rng, "s%d" % i, int(start[i]), int(length[i]), rc=i & 1, seg="afbn"[i % 4])
    return m


def make_empty():
    return _blank("empty", 120, ms.Rng(7003), {60: 2})


def make_gaps0():
    m = make_shapes()
    m.ref_id = "gaps0"
    m.gaps[0] = 2
    return m


def fixture_text(name):
    with open(os.path.join(ms.GOLDEN, "maln", name), encoding="latin1") as f:
        return f.read()


def make_case(name):
    if name in FIXTURES:
        return ms.parse_maln(fixture_text(name))
    if name in SYNTH:
        m = copy.deepcopy(ms.make_case(name))
        m.gaps[0] = 0
        return m
    if name in SCAN_EDGES:
        return make_records(int(name[5:]))
    return {"shapes": make_shapes, "column300": make_column300, "empty": make_empty, "gaps0": make_gaps0}[name]()


def case_text(name):
    """the .maln from its MALN_NAS line on"""
    return fixture_text(name) if name in FIXTURES else ms.write_maln(make_case(name))
