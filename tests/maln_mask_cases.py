"""The .maln files of the end mask (ma_hip -E, -x, -f 96; MiaHip.ma_mask): the smallest shapes at which the kernels of
csrc/mia_ma_mask_kernels.h can go wrong.  Rebuilt from fixed seeds on maln_synth's Maln and writer; nothing here is committed as text.

  empty        no record (no launch)
  one_col      one record of one column
  ones16       sixteen records of one column: all inside one lane's stretch of 16 flat positions
  offsets      300 records of 1 .. 40 columns with '-' columns and inserts: a record begins and ends on every offset of a stretch
  chunk_edge   a record of 40 columns over flat positions 4 080 .. 4 119 (a workgroup's chunk ends at 4 095), short ones around it
  long_5000    one record of 5 000 columns, MIDDLE codes inside it, a zone code in its middle, and a short one behind it
  all_emptied  records of 1 .. 14 columns: under (15, 15) every one is emptied
  pairs300     a record of 400 columns with 300 pairs, among them pairs at 0, at a, at a + 1, at b - 1, at b and at n for (3, 3)
  dashes       '-' at either boundary, runs of '-', '-' columns with zone codes behind the zone, a record of '-' alone, a bad code on a
               '-' column, lower-case bases
  codes        400 records with any code anywhere (zone codes between kept columns), 6 % '-' columns, both strands, inserts
"""
import numpy as np

import maln_ace_cases as mc
import maln_synth as ms

CASES = ("empty", "one_col", "ones16", "offsets", "chunk_edge", "long_5000", "all_emptied", "pairs300", "dashes", "codes")
CHUNK = 4096                                                 # flat positions of a workgroup of k_ma_mask_bounds
_made = {}


def add(m, rid, start, seq, rc=0, smp=None, ins=(), seg="n"):
    n = len(seq)
    m.rec.append({"id": rid, "desc": "", "score": 100 + len(m.rec), "num_inputs": 1, "start": int(start), "end": int(start) + n - 1, "rc": int(rc), "tr": 0, "dr": 0,
                  "seg": seg, "seq": seq, "smp": mc._smp(n) if smp is None else smp, "ins": list(ins)})


def drawn(m, rng, rid, start, n, rc=0, dash=0.03, ins=0, smp=None):
    """the reference's columns with a few other bases and '-' columns, `ins` pairs at random positions 0 .. n"""
    ref = np.frombuffer(m.ref_seq[start:start + n].encode(), np.uint8)
    u = rng.random(n)
    seq = np.where(u < 0.04, mc.ACGT[rng.integers(0, 4, n)], ref)
    seq = np.where((u >= 0.04) & (u < 0.04 + dash), ord("-"), seq).astype(np.uint8).tobytes().decode()
    pairs = sorted((int(p), "ACGT"[int(p) % 4] * (1 + int(p) % 3)) for p in set(rng.integers(0, n + 1, ins).tolist())) if ins else []
    add(m, rid, start, seq, rc, smp, pairs)
    for p, s in pairs:
        if 0 < p < n:
            m.gaps[start + p] = max(m.gaps[start + p], len(s))


def make(name):
    seed = 9800 + CASES.index(name)
    rng = ms.Rng(seed)
    m = mc._blank(name, 6000 if name == "long_5000" else 700, rng, {})
    if name == "one_col":
        add(m, "r0", 5, m.ref_seq[5])
    elif name == "ones16":
        for k in range(16):
            add(m, "r%d" % k, 3 * k, "-" if k == 7 else m.ref_seq[3 * k], rc=k & 1, smp="AP_"[k % 3])
    elif name == "offsets":
        lens, starts, rcs = rng.integers(1, 41, 300), rng.integers(0, 600, 300), rng.integers(0, 2, 300)
        for k in range(300):
            drawn(m, rng, "r%d" % k, starts[k], int(lens[k]), int(rcs[k]), ins=int(k % 4 == 0) * 3)
    elif name == "chunk_edge":
        total = 0
        k = 0
        while total < CHUNK - 16:
            n = min(int(rng.integers(20, 60, 1)[0]), CHUNK - 16 - total)
            drawn(m, rng, "r%d" % k, int(rng.integers(0, 600, 1)[0]), n, k & 1)
            total += n
            k += 1
        drawn(m, rng, "straddle", 100, 40, 0, ins=4)
        drawn(m, rng, "behind", 200, 35, 1)
    elif name == "long_5000":
        code = list(mc._smp(5000))
        code[2500] = "C"                                     # a 5' zone code between kept columns
        drawn(m, rng, "long", 10, 5000, 0, ins=20, smp="".join(code))
        drawn(m, rng, "short", 40, 37, 1)
    elif name == "all_emptied":
        for k in range(60):
            drawn(m, rng, "r%d" % k, 10 * k, 1 + k % 14, k & 1, ins=k % 3)
    elif name == "pairs300":
        n = 400
        seq = m.ref_seq[20:20 + n]
        at = sorted(set([0, 3, 4, 5, 396, 397, 398, 400] + (6 + rng.permutation(380)[:292]).tolist()))
        pairs = [(p, "ACGT"[p % 4] * (1 + p % 2)) for p in at]
        add(m, "many", 20, seq, 0, None, pairs)
        for p, s in pairs:
            if 0 < p < n:
                m.gaps[20 + p] = max(m.gaps[20 + p], len(s))
        drawn(m, rng, "other", 30, 50, 1, ins=2)
    elif name == "dashes":
        r = m.ref_seq
        s40 = mc._smp(40)
        add(m, "d_front", 0, r[0:3] + "-" + r[4:40])                                   # (3, 3): a = 4
        add(m, "d_back", 0, r[0:36] + "-" + r[37:40], rc=1)                            # (3, 3): b = 36
        add(m, "d_runs", 0, r[0:3] + "----" + r[7:33] + "----" + r[37:40])
        add(m, "d_zone_dash", 0, r[0:3] + "-" + "-" + r[5:40], smp=s40[:4] + "B" + s40[5:])   # a '-' with a zone code behind a stripped '-'
        add(m, "d_only", 0, r[0:3] + "-" * 34 + r[37:40])                              # emptied by the boundary rule
        add(m, "d_all", 50, "-" * 12, smp="P" * 12)
        add(m, "d_bad", 0, r[0:3] + "-" + r[4:40], smp=s40[:3] + "~" + s40[4:])       # the bad code is in no zone: stripped
        add(m, "d_lower", 0, r[0:40].lower(), rc=1)
        add(m, "d_inner", 0, r[0:20] + "-" + r[21:40], ins=[(4, "A"), (20, "C"), (36, "G"), (37, "T")])
        m.gaps[4] = m.gaps[20] = m.gaps[36] = m.gaps[37] = 1
    elif name == "codes":
        lens, starts, rcs = rng.integers(1, 90, 400), rng.integers(0, 600, 400), rng.integers(0, 2, 400)
        for k in range(400):
            n = int(lens[k])
            smp = (rng.integers(0, 31, n) + ord("A")).astype(np.uint8).tobytes().decode()
            drawn(m, rng, "r%d" % k, starts[k], n, int(rcs[k]), dash=0.06, ins=int(k % 5 == 0) * 4, smp=smp)
    if name in ("offsets", "codes"):
        m.rec.sort(key=lambda r: (r["start"], r["end"]))
    return m


def case(name):
    if name not in _made:
        _made[name] = make(name)
    return _made[name]
