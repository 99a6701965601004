"""Synthetic .maln files for the ma / insert / consensus kernels, and a numpy reading of what the reference's `ma` does with them.

Three parts, plain Python and numpy, shared by tools/make_ma_synth_goldens.py and the tests:

  parse_maln / write_maln   the text format of write_ma (reference src/map_alignment.c:283-382) without its first line (version and
                            time stamp: MA_HEADER stands in for it), byte for byte
  CASES / make_case         a deterministic generator: the cases of tests/golden/ma_synth/runs.json, rebuilt from their seeds (the
                            .maln texts are never committed).  The random numbers are a counter through splitmix64, written out
                            here, so that no library version can move them
  restate                   show_consensus, add_base, find_ins_cons, find_consensus, find_phred_qscore, show_single_pos and
                            fasta_print_cons (src/map_alignment.c:107-220, src/map_align.c:152-391,444-510, src/io.c:929-951) in
                            int64: every column's ten words, the records that span each column, every insert slot's nine words, the
                            -f 41 / -f 4 tables and the -f 5 sequence.  tests/test_ma_synth_cpu.py holds it against the recorded
                            output of the reference itself, so that a GPU test can name the column and the word that differ
"""
import hashlib
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
MA_HEADER = "/* map_alignment [V1.0] */ golden\n"
PSSM_DEPTH = 15
FASTA_LINE_WIDTH = 60
COL_WORDS = ("A", "C", "G", "T", "gaps", "cov", "scoreA", "scoreC", "scoreG", "scoreT")        # rows of Restated.cols, words 0..9 of the GPU tally
INS_WORDS = ("A", "C", "G", "T", "bases", "scoreA", "scoreC", "scoreG", "scoreT")              # columns of Restated.ins
INT_MIN = -2147483648


# ---- the text format -------------------------------------------------------------------------------------------------------
class Maln:
    """What write_ma writes, field by field.  Per record: id, desc, score, num_inputs (None: no such line), start, end, rc, tr,
    dr (None: no such line), seg, seq, smp, ins [(position in the record, string)]."""

    def __init__(self):
        self.siz = 0
        self.coc = 1
        self.ref_id = ""
        self.ref_desc = ""
        self.L = 0
        self.size = 0
        self.ref_seq = ""
        self.gaps = np.zeros(0, np.int32)
        self.depth = PSSM_DEPTH
        self.fpsm = np.zeros((2 * PSSM_DEPTH + 1, 5, 5), np.int32)
        self.rpsm = np.zeros((2 * PSSM_DEPTH + 1, 5, 5), np.int32)
        self.rec = []


def _after(line, key):
    assert line.startswith(key), (key, line[:40])
    return line[len(key):]


def parse_maln(text):
    """the text of a .maln from its MALN_NAS line on"""
    lines = text.split("\n")
    assert lines[-1] == "", "a .maln ends in a newline"
    k = 0

    def nxt():
        nonlocal k
        k += 1
        return lines[k - 1]

    m = Maln()
    nas = int(_after(nxt(), "MALN_NAS "))
    m.siz = int(_after(nxt(), "MALN_SIZ "))
    m.coc = int(_after(nxt(), "MALN_COC "))
    assert nxt() == "__REFERENCE__"
    m.ref_id = _after(nxt(), "ID ")
    m.ref_desc = _after(nxt(), "DESC ")
    m.L = int(_after(nxt(), "LEN "))
    m.size = int(_after(nxt(), "SIZE "))
    m.ref_seq = _after(nxt(), "SEQ ")
    m.gaps = np.array(_after(nxt(), "GAPS").split(), dtype=np.int32)
    assert len(m.ref_seq) == m.L == len(m.gaps)
    assert nxt() == "__PSSM__"
    m.depth = int(_after(nxt(), "DEPTH "))
    for label, sm in (("FPSM:", m.fpsm), ("RPSM:", m.rpsm)):
        assert nxt() == label
        for d in range(2 * m.depth + 1):
            for row in range(5):
                sm[d, row] = [int(x) for x in nxt().split(" ")]
            assert nxt() == ""
    assert nxt() == "__ALNSEQS__"
    for _ in range(nas):
        r = {"id": _after(nxt(), "ID "), "desc": _after(nxt(), "DESC "), "score": int(_after(nxt(), "SCORE ")), "num_inputs": None, "dr": None}
        line = nxt()
        if line.startswith("NUM_INPUTS "):
            r["num_inputs"] = int(_after(line, "NUM_INPUTS "))
            line = nxt()
        r["start"] = int(_after(line, "START "))
        r["end"] = int(_after(nxt(), "END "))
        r["rc"] = int(_after(nxt(), "RC "))
        r["tr"] = int(_after(nxt(), "TR "))
        line = nxt()
        if line.startswith("DR "):
            r["dr"] = int(_after(line, "DR "))
            line = nxt()
        r["seg"] = _after(line, "SEG ")
        r["seq"] = _after(nxt(), "SEQ ")
        r["smp"] = _after(nxt(), "SMP ")
        tok = _after(nxt(), "INS_POS").split()
        r["ins"] = [(int(tok[i]), tok[i + 1]) for i in range(0, len(tok), 2)]
        m.rec.append(r)
    assert k == len(lines) - 1, "text behind the last record"
    return m


def write_maln(m):
    """the inverse of parse_maln"""
    out = ["MALN_NAS %d\nMALN_SIZ %d\nMALN_COC %d\n__REFERENCE__\nID %s\nDESC %s\nLEN %d\nSIZE %d\nSEQ %s\nGAPS" %
           (len(m.rec), m.siz, m.coc, m.ref_id, m.ref_desc, m.L, m.size, m.ref_seq)]
    out.append("".join(" %d" % g for g in m.gaps.tolist()))
    out.append("\n__PSSM__\nDEPTH %d\n" % m.depth)
    for label, sm in (("FPSM:\n", m.fpsm), ("RPSM:\n", m.rpsm)):
        out.append(label)
        for d in range(2 * m.depth + 1):
            for row in range(5):
                out.append("%d %d %d %d %d\n" % tuple(sm[d, row].tolist()))
            out.append("\n")
    out.append("__ALNSEQS__\n")
    for r in m.rec:
        out.append("ID %s\nDESC %s\nSCORE %d\n" % (r["id"], r["desc"], r["score"]))
        if r["num_inputs"] is not None:
            out.append("NUM_INPUTS %d\n" % r["num_inputs"])
        out.append("START %d\nEND %d\nRC %d\nTR %d\n" % (r["start"], r["end"], r["rc"], r["tr"]))
        if r["dr"] is not None:
            out.append("DR %d\n" % r["dr"])
        out.append("SEG %s\nSEQ %s\nSMP %s\nINS_POS" % (r["seg"], r["seq"], r["smp"]))
        out.append("".join(" %d %s" % (p, s) for p, s in r["ins"]))
        out.append("\n")
    return "".join(out)


def flatten(m):
    """the records as MiaHip.ma_tally takes them (file order; columns START .. END of SEQ and SMP)"""
    n = len(m.rec)
    start = np.array([r["start"] for r in m.rec], np.int32).reshape(n)
    ncols = np.array([r["end"] - r["start"] + 1 for r in m.rec], np.int64).reshape(n)
    col_off = np.zeros(n + 1, np.int64)
    np.cumsum(ncols, out=col_off[1:])
    seq = np.frombuffer("".join(r["seq"][:c] for r, c in zip(m.rec, ncols.tolist())).encode("latin1"), np.uint8)
    smp = np.frombuffer("".join(r["smp"][:c] for r, c in zip(m.rec, ncols.tolist())).encode("latin1"), np.uint8)
    assert len(seq) == len(smp) == col_off[-1]
    ins_record, ins_pos, ins_len, ins_str = [], [], [], []
    for i, r in enumerate(m.rec):
        for p, s in r["ins"]:
            ins_record.append(i)
            ins_pos.append(p)
            ins_len.append(len(s))
            ins_str.append(s)
    ins_off = np.zeros(len(ins_len) + 1, np.int64)
    np.cumsum(np.array(ins_len, np.int64), out=ins_off[1:])
    return {"L": m.L, "gaps": m.gaps.astype(np.int32), "start": start, "revcom": np.array([1 if r["rc"] else 0 for r in m.rec], np.uint8).reshape(n),
            "col_off": col_off, "seq": seq, "smp": smp, "ins_record": np.array(ins_record, np.int32), "ins_pos": np.array(ins_pos, np.int32),
            "ins_off": ins_off, "ins_bases": np.frombuffer("".join(ins_str).encode("latin1"), np.uint8)}


def ma_tally_args(f):
    """flatten()'s arrays in the order of MiaHip.ma_tally's parameters"""
    return (f["L"], f["gaps"], f["start"], f["revcom"], f["col_off"], f["seq"], f["smp"], f["ins_record"], f["ins_pos"], f["ins_off"], f["ins_bases"])


# ---- substitution matrices ---------------------------------------------------------------------------------------------------
def flat_pssm():
    """init_flatsubmat (src/pssm.c:96-126)"""
    p = np.zeros((31, 5, 5), np.int32)
    p[:, :4, :4] = -600
    for i in range(4):
        p[:, i, i] = 200
    p[:, :, 4] = -100
    p[:, 4, :] = -10
    return p


def read_pssm(path):
    """read_pssm (src/io.c:408-503): 31 blocks of a title line, four rows of four tab-separated numbers and a blank line"""
    p = np.zeros((31, 5, 5), np.int32)
    lines = open(path).read().split("\n")
    for d in range(31):
        assert "# Matrix for position" in lines[6 * d], path
        for i in range(4):
            p[d, i, :4] = [int(x) for x in lines[6 * d + 1 + i].split("\t")[:4]]
    p[:, :4, 4] = -100
    p[:, 4, :] = -10
    return p


def revcom_pssm(p):
    """revcom_submat (src/pssm.c:53-91): rc[30 - d][3 - i][3 - j] = sm[d][i][j], index 4 stays"""
    idx = np.array([3, 2, 1, 0, 4])
    return np.ascontiguousarray(p[::-1][:, idx][:, :, idx]).astype(np.int32)


def matrix(name):
    return flat_pssm() if name == "flat" else read_pssm(os.path.join(GOLDEN, name))


# ---- the reference's arithmetic, restated -----------------------------------------------------------------------------------
_CODE = np.full(256, 4, np.int64)          # base2inx (src/map_align.c:16-29): everything that is no base is column 4
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _i
GAP = ord("-")


def find_consensus(A, C, G, T, gaps, cov, sA, sC, sG, sT, cons_code):
    """find_consensus (src/map_align.c:294-391): (call, frac_agree)"""
    if cov == 0:
        return "N", 0.0
    if gaps / cov >= 50 / 100.0:
        return "-", gaps / cov
    top, second, base, frac = sA, INT_MIN, "A", A / cov
    if sC >= top:
        second, top, base, frac = top, sC, "C", C / cov
    else:
        second = sC
    if sG >= top:
        second, top, base, frac = top, sG, "G", G / cov
    elif sG >= second:
        second = sG
    if sT >= top:
        second, top, base, frac = top, sT, "T", T / cov
    elif sT >= second:
        second = sT
    if cons_code == 2:
        return (base if (top >= 0 or top - 2400 > second) else "N"), frac
    return (base if top >= -399 else "N"), frac


def _pow2(x):
    try:
        return math.pow(2.0, x)
    except OverflowError:
        return math.inf


def find_phred_qscore(sA, sC, sG, sT):
    """find_phred_qscore (src/map_align.c:152-206), the conversion to int as x86-64 does it (not a number, or out of range: INT_MIN)"""
    if sA >= sC and sA >= sG and sA >= sT:
        best, rest = sA, (sC, sG, sT)
    elif sC >= sG and sC >= sT:
        best, rest = sC, (sA, sG, sT)
    elif sG >= sT:
        best, rest = sG, (sA, sC, sT)
    else:
        best, rest = sT, (sA, sC, sG)
    pb = _pow2(best / 100)
    den = _pow2(rest[0] / 100) + _pow2(rest[1] / 100) + _pow2(rest[2] / 100)
    if den == 0.0:
        pc = math.nan if pb == 0.0 else math.inf
    elif math.isinf(pb) and math.isinf(den):
        pc = math.nan
    else:
        pc = pb / den
    if pc >= 1.7976931348623157e308:
        pc = 1.7976931348623157e308
    if math.isnan(pc) or pc <= 0.0:
        return INT_MIN
    v = 10 * math.log10(pc)
    return int(v) if abs(v) < 2147483648.0 else INT_MIN


class Restated:
    """cols[10][L] (COL_WORDS), span[L] (records with START < p <= END), ins_off[L + 1] (ins_off[p] = GAPS[1] + .. + GAPS[p - 1]),
    ins[slots][9] (INS_WORDS), all int64"""

    def __init__(self, f, fpsm, rpsm, ref_seq, ref_id):
        L = f["L"]
        self.L, self.ref_seq, self.ref_id = L, ref_seq, ref_id
        self.gaps = f["gaps"].astype(np.int64)
        start, col_off = f["start"].astype(np.int64), f["col_off"]
        n = len(start)
        ncols = col_off[1:] - col_off[:-1]
        assert n == 0 or (start.min() >= 0 and (start + ncols).max() <= L), "a record outside the reference"
        psm = np.stack([fpsm, rpsm]).astype(np.int64)                    # [strand][depth][row][column]
        rec = np.repeat(np.arange(n), ncols)
        col = start[rec] + (np.arange(col_off[-1]) - col_off[:-1][rec])
        # show_consensus / add_base, src/map_alignment.c:154-169, src/map_align.c:229-263
        self.cols = np.zeros((10, L), np.int64)
        code, depth, strand = _CODE[f["seq"]], f["smp"].astype(np.int64) - ord("A"), f["revcom"].astype(np.int64)[rec]
        is_gap = f["seq"] == GAP
        assert ((depth >= 0) & (depth <= 2 * PSSM_DEPTH))[~is_gap].all(), "a depth code outside A.._"
        for b in range(4):
            self.cols[b] = np.bincount(col[(code == b) & ~is_gap], minlength=L)
        self.cols[4] = np.bincount(col[is_gap], minlength=L)
        self.cols[5] = np.bincount(col, minlength=L)
        k = ~is_gap
        for row in range(4):
            np.add.at(self.cols[6 + row], col[k], psm[strand[k], depth[k], row, code[k]])
        # find_ins_cons, src/map_align.c:463-495: the records with START < pos <= END
        d = np.zeros(L + 2, np.int64)
        np.add.at(d, start + 1, 1)
        np.add.at(d, start + ncols, -1)
        self.span = np.cumsum(d)[:L]
        self.ins_off = np.zeros(L + 1, np.int64)
        if L > 1:
            np.cumsum(self.gaps[1:], out=self.ins_off[2:])
        slots = int(self.ins_off[L])
        self.ins = np.zeros((slots, 9), np.int64)
        ir, ip, io, ib = f["ins_record"].astype(np.int64), f["ins_pos"].astype(np.int64), f["ins_off"], f["ins_bases"]
        if len(ir):
            assert not (ib == GAP).any(), "a '-' inside an insert string: not covered"
            ilen = io[1:] - io[:-1]
            ev = np.repeat(np.arange(len(ir)), ilen)                     # one element per inserted character
            j = np.arange(io[-1]) - io[:-1][ev]
            r, p = ir[ev], ip[ev]
            gc = start[r] + p
            counted = (p > 0) & (p < ncols[r])
            counted &= j < self.gaps[np.where(counted, gc, 0)]
            ev, j, r, p, gc = ev[counted], j[counted], r[counted], p[counted], gc[counted]
            sl = self.ins_off[gc] + j
            c2, d2, s2 = _CODE[ib[io[:-1][ev] + j]], f["smp"].astype(np.int64)[col_off[:-1][r] + p] - ord("A"), f["revcom"].astype(np.int64)[r]
            for b in range(4):
                self.ins[:, b] = np.bincount(sl[c2 == b], minlength=slots)
            self.ins[:, 4] = np.bincount(sl, minlength=slots)
            for row in range(4):
                np.add.at(self.ins[:, 5 + row], sl, psm[s2, d2, row, c2])
        self.slot_col = np.repeat(np.arange(L), np.where(np.arange(L) > 0, self.gaps, 0))      # column of every slot

    def col_counts(self, p):
        return tuple(int(x) for x in self.cols[:, p])

    def slot_counts(self, s):
        """an insert slot as find_consensus sees it: a record that spans the column without a base there adds a gap"""
        t, span = self.ins[s], int(self.span[self.slot_col[s]])
        return (int(t[0]), int(t[1]), int(t[2]), int(t[3]), span - int(t[4]), span, int(t[5]), int(t[6]), int(t[7]), int(t[8]))

    def calls(self, cons_code):
        """(call of every column, call of every insert slot)"""
        return ("".join(find_consensus(*self.col_counts(p), cons_code)[0] for p in range(self.L)),
                "".join(find_consensus(*self.slot_counts(s), cons_code)[0] for s in range(len(self.ins))))

    def consensus(self, cons_code):
        """the assembled string: before every column but the first its insert slots, '-' left out (src/io.c:936)"""
        cc, ic = self.calls(cons_code)
        out = []
        for p in range(self.L):
            if p > 0 and self.gaps[p] > 0:
                out.append(ic[self.ins_off[p]:self.ins_off[p] + self.gaps[p]])
            out.append(cc[p])
        return "".join(out).replace("-", "")

    def f5(self, cons_code):
        s = self.consensus(cons_code)
        full = len(s) // FASTA_LINE_WIDTH * FASTA_LINE_WIDTH
        return ">%s\n" % self.ref_id + "".join(s[i:i + FASTA_LINE_WIDTH] + "\n" for i in range(0, full, FASTA_LINE_WIDTH)) + s[full:] + "\n"

    @staticmethod
    def _line(p, ref_base, b, cons_code):
        A, C, G, T, gaps, cov, sA, sC, sG, sT = b
        call, frac = find_consensus(*b, cons_code)
        return call, "%d %s %s %d %d %d %d %d %d %d %d %d %d %d %0.3f\n" % (p, ref_base, call, cov, A, C, G, T, gaps, sA, sC, sG, sT,
                                                                             find_phred_qscore(sA, sC, sG, sT), frac)

    def table(self, cons_code, fmt=41):
        """-f 41: a line per insert slot and per column (show_single_pos, src/map_align.c:208-227); -f 4: only where the call differs"""
        out = []
        for p in range(self.L):
            if p > 0:
                for s in range(int(self.ins_off[p]), int(self.ins_off[p] + self.gaps[p])):
                    call, line = self._line(p, "-", self.slot_counts(s), cons_code)
                    if fmt == 41 or call != "-":
                        out.append(line)
            call, line = self._line(p, self.ref_seq[p], self.col_counts(p), cons_code)
            if fmt == 41 or call != self.ref_seq[p]:
                out.append(line)
        return "".join(out)

    def output(self, key):
        """the reference's stdout for a run key "f<format>c<code>" """
        fmt, code = key[1:].split("c")
        return self.f5(int(code)) if fmt == "5" else self.table(int(code), int(fmt))


def restate(m):
    return Restated(flatten(m), m.fpsm, m.rpsm, m.ref_seq, m.ref_id)


# ---- the generator -------------------------------------------------------------------------------------------------------------
class Rng:
    """splitmix64 over a counter"""

    def __init__(self, seed):
        self.seed, self.k = seed, 0

    def u64(self, n):
        z = (np.arange(self.k, self.k + n, dtype=np.uint64) + np.uint64(self.seed * 1000003 + 1)) * np.uint64(0x9E3779B97F4A7C15)
        self.k += n
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))

    def integers(self, lo, hi, n):
        """n values in lo .. hi - 1"""
        return (self.u64(n) % np.uint64(hi - lo)).astype(np.int64) + lo

    def random(self, n):
        return (self.u64(n) >> np.uint64(11)).astype(np.float64) / float(1 << 53)

    def permutation(self, n):
        return np.argsort(self.u64(n), kind="stable")


RUN_KEYS = ("f41c1", "f41c2", "f5c1", "f5c2", "f4c1")

# Slot specs of an insert column, one per gap position: (how many of the S spanning records have a base there, dominant base,
# share of N among the bases).  "half": exactly S / 2 (S is made even), "under": S / 2 + 1 -- one gap short of the 50 % that call '-'.
DEEP_INS = {
    4070: [(0.80, "C", 0.0), (0.70, "A", 0.0), ("under", "G", 0.0)],        # C-heavy: scoreA < 0 <= scoreC; A-heavy: the other way round
    4075: [(0.90, "T", 0.0), ("half", "G", 0.0)],
    4080: [(0.80 - 0.06 * j, "ACGT"[j % 4], 0.02) for j in range(12)],      # 80 % .. 14 %: the tail calls '-'
    4085: [(0.80, "A", 0.72)],                                             # N under code 1 (top score < -399), A under code 2 (2400 ahead)
    4090: [(0.75, "G", 0.0), (0.70, "T", 0.0), (0.65, "G", 0.05), (0.60, "T", 0.0), (0.55, "C", 0.0)],
    4096: [(0.85, "A", 0.0), (0.60, "C", 0.0)],
}
CASES = {
    "one_col": dict(seed=11, L=1, n=3, matrix="flat", lens=(1, 1)),
    "edge255": dict(seed=12, L=255, n=300, matrix="flat", lens=(1, 256), ins={1: [(0.9, "A", 0.0), (0.4, "C", 0.0)], 254: [(0.8, "G", 0.0)]}, pos0=True),
    "edge256": dict(seed=13, L=256, n=300, matrix="ancient.submat.txt", lens=(1, 256),
                    ins={1: [(0.9, "C", 0.0)], 254: [(0.8, "T", 0.0), ("half", "A", 0.0)], 255: [(0.7, "G", 0.0), (0.6, "A", 0.0), (0.2, "C", 0.0)]}, pos0=True),
    "edge257": dict(seed=14, L=257, n=300, matrix="ancient.submat.solexa.pe.txt", lens=(1, 256),
                    ins={1: [(0.9, "G", 0.0)], 254: [(0.8, "A", 0.0)], 255: [("under", "C", 0.0)], 256: [(0.9, "T", 0.0), (0.7, "T", 0.1)]}, pos0=True),
    # k_excl_scan walks L + 1 elements: its stretch is 256 long up to L = 4095 and 512 from L = 4096 on
    "scan16_4095": dict(seed=15, L=4095, n=4000, matrix="flat", lens=(20, 80), ins={1023: [(0.8, "A", 0.0)], 1024: [(0.8, "C", 0.0), (0.7, "G", 0.0)], 4094: [(0.9, "T", 0.0)]},
                        clusters=((990, 40, 2000), (3955, 110, 2000))),
    "scan16_4096": dict(seed=16, L=4096, n=4000, matrix="ancient.submat.txt", lens=(20, 80),
                        ins={1023: [(0.8, "T", 0.0)], 1024: [(0.9 - 0.02 * j, "ACGT"[(j * 7) % 4], 0.01) for j in range(40)], 4095: [(0.9, "G", 0.0)]},
                        clusters=((990, 40, 2000), (3956, 110, 2000))),
    "scan16_4097": dict(seed=17, L=4097, n=4000, matrix="flat", lens=(20, 80),
                        ins={1023: [(0.8, "G", 0.0)], 1024: [(0.8, "A", 0.0)], 4095: [(0.7, "C", 0.0), ("half", "T", 0.0)], 4096: [(0.9, "A", 0.0)]},
                        clusters=((990, 40, 2000), (3957, 110, 2000))),
    "deep": dict(seed=18, L=9000, n=20000, matrix="ancient.submat.solexa.pe.txt", lens=(30, 256), ins=DEEP_INS, clusters=((4000, 60, 9000), (100, 200, 5500), (8000, 200, 5500))),
    "codes_anc": dict(seed=19, L=600, n=2000, matrix="ancient.submat.txt", lens=(2, 100), ins={300: [(0.8, "C", 0.05), (0.6, "A", 0.05)]}, all_codes=True, clusters=((100, 60, 2000),)),
    "codes_flat": dict(seed=20, L=600, n=2000, matrix="flat", lens=(2, 100), ins={300: [(0.8, "G", 0.05), (0.6, "T", 0.05)]}, all_codes=True, clusters=((100, 60, 2000),)),
}
BIG_CASES = ("deep",)                      # their -f 41 outputs are files of their own under tests/golden/ma_synth


def make_case(name):
    """the Maln of a case of CASES"""
    c = CASES[name]
    rng, L, n = Rng(c["seed"]), c["L"], c["n"]
    lo, hi = c["lens"]
    acgt = np.frombuffer(b"ACGT", np.uint8)
    ref = acgt[rng.integers(0, 4, L)]
    ncols = np.minimum(rng.integers(lo, hi + 1, n), L)
    start = (rng.random(n) * (L - ncols + 1)).astype(np.int64)
    q = 0
    for at, width, k in c.get("clusters", ()):       # the next k records start within `width` columns of `at`: the columns between the
        start[q:q + k] = np.minimum(at + rng.integers(0, width, k), L - ncols[q:q + k])      # clusters stay empty (calls of N, short lines)
        q += k
    if c.get("all_codes"):                 # records of one column and of 256 columns
        ncols[:8], ncols[8:16] = 1, 256
        start[:16] = np.minimum(start[:16], L - ncols[:16])
    ins = c.get("ins", {})
    # every insert column: records that start on it (they do not count, START < pos), that end on it, that start just before it
    q = 16
    for col in sorted(ins):
        for want in ("start", "end", "before"):
            for _ in range(3):
                if want == "start":
                    start[q] = col
                    ncols[q] = min(ncols[q], L - col)
                elif want == "end":
                    ncols[q] = min(ncols[q], col + 1)
                    start[q] = col + 1 - ncols[q]
                else:
                    start[q] = col - 1
                    ncols[q] = max(2, min(ncols[q], L - col + 1))
                q += 1
    assert q <= n or not ins
    # a "half" or "under" slot wants an even number of spanning records: a record of two columns ending on the column makes it so
    for col in sorted(ins):
        if any(s[0] in ("half", "under") for s in ins[col]) and int(((start < col) & (start + ncols > col)).sum()) % 2:
            start, ncols = np.append(start, col - 1), np.append(ncols, 2)
    n = len(start)
    assert (start >= 0).all() and (start + ncols <= L).all() and (ncols >= 1).all()
    cover = np.zeros(L + 1, np.int64)
    np.add.at(cover, start, 1)
    np.add.at(cover, start + ncols, -1)
    ref = np.where(np.cumsum(cover)[:L] > 0, ref, ord("N")).astype(np.uint8)      # N where no record lies: -f 4 has no line there
    rc = (rng.u64(n) & np.uint64(1)).astype(np.int64)
    col_off = np.zeros(n + 1, np.int64)
    np.cumsum(ncols, out=col_off[1:])
    total = int(col_off[-1])
    rec = np.repeat(np.arange(n), ncols)
    off = np.arange(total) - col_off[:-1][rec]
    # SEQ: the reference with 3 % other bases, 1 % N, 2 % '-'
    seq = ref[start[rec] + off].copy()
    u = rng.random(total)
    other = acgt[rng.integers(0, 4, total)]
    seq = np.where(u < 0.03, other, seq)
    seq = np.where((u >= 0.03) & (u < 0.04), ord("N"), seq)
    seq = np.where((u >= 0.04) & (u < 0.06), GAP, seq).astype(np.uint8)
    # SMP: distance from the nearer end, as pop_smp_from_FSDB writes it (src/fsdb.c:572-582) -- or any code anywhere
    back = ncols[rec] - 1 - off
    smp = np.where(off < PSSM_DEPTH, off, np.where(back < PSSM_DEPTH, 2 * PSSM_DEPTH - back, PSSM_DEPTH))
    if c.get("all_codes"):
        smp = rng.integers(0, 2 * PSSM_DEPTH + 1, total)
    smp = (smp + ord("A")).astype(np.uint8)
    gaps = np.zeros(L, np.int64)
    inserts = {}                           # (record, position in the record) -> string

    def draw(k, dominant, n_share):
        u = rng.random(k)
        b = np.where(u < 0.88, ord(dominant), acgt[rng.integers(0, 4, k)])
        return np.where(rng.random(k) < n_share, ord("N"), b).astype(np.uint8)

    for col in sorted(ins):
        who = np.nonzero((start < col) & (start + ncols > col))[0]
        S = len(who)
        who = who[rng.permutation(S)]
        counts, prev = [], S
        for share, _, _ in ins[col]:
            k = S // 2 if share == "half" else S // 2 + 1 if share == "under" else int(share * S)
            prev = max(1, min(prev, k))
            counts.append(prev)
        strings = np.zeros((S, len(counts)), np.uint8)
        for j, (k, (_, dominant, n_share)) in enumerate(zip(counts, ins[col])):
            strings[:k, j] = draw(k, dominant, n_share)
        length = (strings != 0).sum(axis=1)
        for i in range(counts[0]):
            inserts[(int(who[i]), int(col - start[who[i]]))] = strings[i, :length[i]].tobytes().decode()
        gaps[col] = len(counts)
    # stray inserts of 1 .. 3 bases, one record each: most of these columns call '-' and leave the string alone
    n_stray = n // 20 if L > 8 else 0
    sr, su, sl = rng.integers(0, n, n_stray), rng.random(n_stray), rng.integers(1, 4, n_stray)
    sb = acgt[rng.integers(0, 4, 3 * n_stray)].tobytes().decode()
    for t in range(n_stray):
        r = int(sr[t])
        if ncols[r] < 2:
            continue
        p = 1 + int(su[t] * (ncols[r] - 1))
        col = int(start[r]) + p
        if col in ins or (r, p) in inserts:
            continue
        inserts[(r, p)] = sb[3 * t:3 * t + int(sl[t])]
        gaps[col] = max(gaps[col], int(sl[t]))
    if c.get("pos0"):                      # an insert in front of a record's own first column: never looked at (START < pos)
        for col in sorted(ins):
            for r in np.nonzero(start == col)[0][:2].tolist():
                inserts[(r, 0)] = "ACGT"[r % 4] * int(gaps[col])
    gaps[0] = 3                            # the reference skips column 0 whatever GAPS says
    m = Maln()
    m.siz = 16000
    while m.siz < n:
        m.siz *= 2
    m.ref_id, m.ref_desc, m.L, m.size, m.ref_seq, m.gaps = name, "", L, 2 * L + 2, ref.tobytes().decode(), gaps.astype(np.int32)
    m.fpsm = matrix(c["matrix"])
    m.rpsm = revcom_pssm(m.fpsm)
    seq_s, smp_s = seq.tobytes().decode("latin1"), smp.tobytes().decode("latin1")
    by_rec = {}
    for (r, p), s in inserts.items():
        by_rec.setdefault(r, []).append((p, s))
    for i in range(n):
        a, b = int(col_off[i]), int(col_off[i + 1])
        m.rec.append({"id": "s%d" % i, "desc": "", "score": 2000 + 7 * i % 5000, "num_inputs": 1, "start": int(start[i]), "end": int(start[i] + ncols[i] - 1),
                      "rc": int(rc[i]), "tr": int(i % 11 == 0), "dr": int(i % 13 == 0), "seg": "n", "seq": seq_s[a:b], "smp": smp_s[a:b],
                      "ins": sorted(by_rec.get(i, []))})
    return m


def maln_sha256(m):
    return hashlib.sha256(write_maln(m).encode("latin1")).hexdigest()
