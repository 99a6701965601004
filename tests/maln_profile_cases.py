"""The .maln files of the substitution profile (ma_hip -f 9, -f 91) that no other module makes: the smallest shapes at which
k_ma_profile can go wrong.  Rebuilt from fixed seeds on maln_synth's Maln and writer; nothing here is committed as text.

The kernel walks the FLAT columns -- the records' SEQ / SMP strings end to end, T characters -- and these are its constants
(csrc/ma_profile_body.h, csrc/mia_ma_profile_kernels.h):
  LANE = 16      flat positions a lane takes at a time (one 16-byte load; the record of the first is found by bisection, the rest
                 by walking on)
  WAVE = 1 024   flat positions of a wavefront's 64 lanes
  WG   = 4 096   flat positions of a workgroup's chunk; the grid strides over the chunks
  hot bins       (MIDDLE, X, X): counted by ballot into registers, every other bin by an LDS atomic on 32-bit words

  prof_classes        240 records of 40 .. 60 columns, half of them RC, natural SMP codes (every code 0 .. 30 in every record): every
                      pair of a reference class and a read class (A C G T other) and '-' under every reference class at every depth
                      code on each strand; lower case, N and IUPAC codes in ref_seq and SEQ; every ninth record marked DR
  prof_one_bin        280 forward records of 256 columns, all A on A at code P: 71 680 events in (MIDDLE, A, A) and none elsewhere
  prof_edges_<T>      T flat columns, T = 1, 15, 16, 17, 63, 64, 65, 1 023, 1 024, 1 025, 4 095, 4 096, 4 097: one below, at and
                      above LANE, the 64 of a wavefront, WAVE and WG.  A record of one column first; records that start exactly on
                      flat 16, 64, 2 048 and 4 096; one of 300 columns over flat 900 .. 1 199 (across a WAVE edge and 19 LANE
                      edges); START in no order; both strands
  prof_tail           records of a circular assembly that end on column L (beyond), with a base and with '-' there; the SMP characters
                      '@', '`' ('A' + 31) and '~' (bad_code) -- on '-' columns, where mia_hip_ma_tally lets them pass (bad_on_base: one
                      on a base, which the tally refuses); a record that is all '-'; records without columns
  prof_empty          no records
  prof_all_dropped    every record marked DR: nothing counts without -A
"""
import copy

import maln_ace_cases as mc
import maln_synth as ms

LANE, WAVE, WG = 16, 1024, 4096
EDGE_T = (1, LANE - 1, LANE, LANE + 1, 63, 64, 65, WAVE - 1, WAVE, WAVE + 1, WG - 1, WG, WG + 1)
CASES = ("prof_classes", "prof_one_bin") + tuple("prof_edges_%d" % t for t in EDGE_T) + ("prof_tail", "prof_empty", "prof_all_dropped")
# what the library-call test takes of them (with the other modules' cases it names)
LIBRARY = ("prof_classes", "prof_one_bin", "prof_edges_%d" % (WG + 1), "prof_tail", "prof_empty")
OTHER = "NnRYKMSWBDHVrykmX."               # class 4: N and IUPAC codes in either case, and what is no code at all


def _rec(m, rid, start, seq, smp=None, rc=0, dr=0):
    n = len(seq)
    m.rec.append({"id": rid, "desc": "", "score": 700 + 11 * len(m.rec), "num_inputs": 1 + len(m.rec) % 3, "start": start, "end": start + n - 1, "rc": rc, "tr": 0,
                  "dr": dr, "seg": "n", "seq": seq, "smp": mc._smp(n) if smp is None else smp, "ins": []})


def _char(rng, cls):
    """a character of class 0 .. 4, '-' for 5; a base in lower case one time in four"""
    if cls == 5:
        return "-"
    if cls == 4:
        return OTHER[int(rng.integers(0, len(OTHER), 1)[0])]
    ch = "ACGT"[cls]
    return ch.lower() if rng.integers(0, 4, 1)[0] == 0 else ch


def make_classes():
    rng = ms.Rng(9001)
    L = 700
    m = mc._blank("prof_classes", L, rng, {350: 2})
    m.ref_seq = "".join(_char(rng, p % 5) for p in range(L))        # the class of column p is p % 5
    k_all = 0
    for n in (40, 47, 53, 60):
        for rc in (0, 1):
            for k in range(30):            # start residue k % 5 fixes the reference class of column c, k // 5 turns the read class
                start = 5 * ((17 * k_all) % ((L - 70) // 5)) + k % 5
                seq = "".join(_char(rng, (k // 5 + c) % 6) for c in range(n))
                _rec(m, "c%d" % k_all, start, seq, rc=rc, dr=int(k_all % 9 == 0))
                k_all += 1
    return m


def make_one_bin():
    rng = ms.Rng(9002)
    m = mc._blank("prof_one_bin", 300, rng, {})
    m.ref_seq = "A" * 300
    for i in range(280):
        _rec(m, "a%d" % i, (7 * i) % 45, "A" * 256, smp="P" * 256)
    return m


def make_edges(T):
    rng = ms.Rng(9100 + T)
    L = 1500
    m = mc._blank("prof_edges_%d" % T, L, rng, {700: 1})
    lens, at = [], 0
    for target in [t for t in (1, LANE, 64, 900, 1200, 2 * WAVE, WG) if t < T] + [T]:
        if (at, target) == (900, 1200):
            lens.append(300)
            at = 1200
        while at < target:
            k = min(int(rng.integers(1, 61, 1)[0]), target - at)
            lens.append(k)
            at += k
    assert sum(lens) == T and lens[0] == 1
    for i, k in enumerate(lens):
        mc._record(m, rng, "e%d" % i, int(rng.integers(0, L - k + 1, 1)[0]), k, rc=i & 1, dash=0.05, dr=int(i % 10 == 3))
    return m


def make_tail():
    rng = ms.Rng(9003)
    L = 500
    m = mc._blank("prof_tail", L, rng, {250: 1})
    ref = lambda s, n: "".join(m.ref_seq[(s + k) % L] for k in range(n))
    _rec(m, "end_L", L - 30, ref(L - 30, 31))
    _rec(m, "end_L_rc", L - 20, ref(L - 20, 21), rc=1)
    _rec(m, "end_L_dash", L - 25, ref(L - 25, 25) + "-", rc=1)
    _rec(m, "end_Lm1", L - 40, ref(L - 40, 40))
    seq, smp = list(ref(100, 50)), list(mc._smp(50))
    for c, code in ((3, "@"), (20, "`"), (21, "~"), (47, "@")):
        seq[c], smp[c] = "-", code
    _rec(m, "bad_codes", 100, "".join(seq), smp="".join(smp))
    _rec(m, "bad_codes_rc", 130, "".join(seq[::-1]), smp="".join(smp[::-1]), rc=1)
    _rec(m, "bad_end_L", L - 3, ref(L - 3, 2) + "--", smp="AB`~")       # column L with a bad code: beyond, and nowhere else
    _rec(m, "only_dashes", 200, "-" * 70)
    _rec(m, "only_dashes_rc", 210, "-" * 33, rc=1)
    _rec(m, "no_columns", 300, "")
    _rec(m, "no_columns_last", 499, "", rc=1)
    for i in range(6):
        mc._record(m, rng, "t%d" % i, 40 * i, 45, rc=i & 1, dr=int(i == 2))
    return m


def bad_on_base():
    """prof_tail with one depth code outside A .. _ on a column that holds a base: mia_hip_ma_tally refuses the file"""
    m = make_tail()
    r = next(r for r in m.rec if r["id"] == "end_Lm1")
    r["smp"] = r["smp"][:5] + "~" + r["smp"][6:]
    return m


def make_all_dropped():
    m = make_edges(65)
    m.ref_id = "prof_all_dropped"
    for r in m.rec:
        r["dr"] = 1
    return m


def make_case(name):
    if name.startswith("prof_edges_"):
        return make_edges(int(name[11:]))
    if name == "prof_empty":
        m = mc.make_empty()
        m.ref_id = "prof_empty"
        return m
    return {"prof_classes": make_classes, "prof_one_bin": make_one_bin, "prof_tail": make_tail, "prof_all_dropped": make_all_dropped}[name]()


def reversed_records(m):
    r = copy.copy(m)
    r.rec = m.rec[::-1]
    return r
