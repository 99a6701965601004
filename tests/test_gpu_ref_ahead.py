"""Reference ahead (csrc/ref_ahead.h): mia_hip_iterate prepares the consensus it returns as the next call's reference,
behind that consensus, into a second set of buffers and the idle half of the control block; a call that brings that string adopts the
set instead of preparing anything.

Two contexts run the same sequence of calls: the default one and one of the alt build made with MIA_HIP_NO_REF_AHEAD=1 (no shadow
launch, every call prepares its own reference).  After every call they must agree on the consensus string, every read's alignment, the
dropped marks, the records' parameters, every tally word and ref->gaps, the insert events and the links -- links() and dropped() fetch
the link count and the cull flags from the device, and tally() runs the step-wise tally again and fetches event count and both flag
words from the device: the twin control block must have left them where the step put them.  Agreement of the two builds is HIP against
HIP, so the first iterations of the circular and of the linear sequence also run beside the oracle (oracle_sample.py).

Shapes: 2 000 - 4 000 synthetic reads of 36 - 100 bases (tools/gen_data.py), references of 600 - 3 000 bases, flat matrix and
ancient.submat.txt -- several workgroups of every kernel, several blocks of k_ref_prep's grid, both sides of its N-column branch."""
import ctypes as C
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import gen_data
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

LENS = (36, 50, 75, 100)


class W:
    pass


def workload(seed, L, n, circular, matrix_file=None, insertion_at=None, hole=None, indel_rate=0.003):
    """reads of LENS drawn from a random genome of L bases; ref0 = that genome with a substitution in one column of a hundred, without
    the two bases at insertion_at (the reads then carry a consistent 2-base insertion), reads kept off the columns of `hole`"""
    import mia_amd
    w = W()
    w.circular, w.matrix_file = circular, matrix_file
    w.pssm = mia_amd.read_pssm(os.path.join(GOLDEN, matrix_file)) if matrix_file else mia_amd.flat_pssm()
    rng = np.random.default_rng(seed)
    genome = gen_data.random_reference(L, seed=seed)
    parts = []
    for k, rl in enumerate(LENS):
        m = n // len(LENS) + (1 if k < n % len(LENS) else 0)
        start = None
        if hole is not None:         # linear: starts on either side of the hole, the read ends before it
            left = rng.integers(0, hole[0] - rl, size=m)
            right = rng.integers(hole[1], L - rl - 8, size=m)
            start = np.where(rng.random(m) < 0.5, left, right)
        d = gen_data.make_reads(genome, m, rl, seed=[seed, rl], circular=circular, damage=matrix_file is not None, indel_rate=indel_rate, start=start)
        parts.append((rl, d, gen_data.stored_orientation(d)))
    w.n = sum(len(d["start"]) for _, d, _ in parts)
    w.stored = np.full((w.n, max(LENS)), ord("A"), np.uint8)
    w.lens = np.concatenate([np.full(len(d["start"]), rl, np.int32) for rl, d, _ in parts])
    at = 0
    for rl, d, st in parts:
        w.stored[at:at + len(st), :rl] = st
        at += len(st)
    w.rc = np.concatenate([d["strand"] for _, d, _ in parts]).astype(np.uint8)
    start = np.concatenate([d["start"] for _, d, _ in parts]).astype(np.int64)
    g = np.frombuffer(genome.encode(), np.uint8).copy()
    cols = rng.choice(L, L // 100, replace=False)
    g[cols] = np.frombuffer(b"ACGT", np.uint8)[(np.searchsorted(np.frombuffer(b"ACGT", np.uint8), g[cols]) + 1) % 4]
    ref0 = g.tobytes().decode()
    if insertion_at is not None:
        ref0 = ref0[:insertion_at] + ref0[insertion_at + 2:]
        start = np.where(start > insertion_at, start - 2, start)
    w.ref0 = ref0
    w.as0 = start.astype(np.int32)
    w.ae0 = (w.as0 + w.lens - 1).astype(np.int32)
    w.sk = np.ones(w.n, np.uint8)
    w.offsets = np.zeros(w.n + 1, np.int64)
    w.offsets[1:] = np.cumsum(w.lens)
    w.flat = np.concatenate([w.stored[i, :w.lens[i]] for i in range(w.n)])
    return w


def context(w, ahead, lo=0, hi=None):
    import mia_amd
    if not ahead:
        os.environ["MIA_HIP_NO_REF_AHEAD"] = "1"
    try:
        h = mia_amd.MiaHip(0)
    finally:
        os.environ.pop("MIA_HIP_NO_REF_AHEAD", None)
    assert h.is_alt_build == (not ahead)
    h.set_pssm(w.pssm)
    upload(h, w, lo, hi)
    return h


def upload(h, w, lo=0, hi=None):
    hi = w.n if hi is None else hi
    h.upload_reads(w.flat[w.offsets[lo]:w.offsets[hi]], w.offsets[lo:hi + 1] - w.offsets[lo], w.rc[lo:hi], w.sk[lo:hi], w.as0[lo:hi], w.ae0[lo:hi])
    h.set_read_base(lo)


class Hip:
    """hipMemcpy through ctypes: insert events and links are handed out as device pointers"""

    def __init__(self):
        self.l = C.CDLL("libamdhip64.so")
        self.l.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]

    def to_host(self, dptr, n, dtype):
        out = np.empty(n, dtype)
        if n:
            assert self.l.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(dptr), out.nbytes, 2) == 0
        return out


def snapshot(h, hipapi, stepwise_tally):
    s = {}
    s["score"], s["as"], s["ae"] = h.alignments()
    s["dropped_f"], s["dropped_b"] = h.dropped()                     # (the cull flags come from the device with them)
    s["params"], s["back_slot"] = h.record_params()
    s["tally"], s["gaps"] = h.get_tally()
    pe, ne = h.ins_events()
    s["events"] = np.sort(hipapi.to_host(pe, ne, np.uint64))        # (appended with atomics: the order is not part of the result)
    pl, nl = h.links()                                               # (the link count comes from the device)
    lk = hipapi.to_host(pl, 4 * nl, np.int64).reshape(-1, 4)
    s["links"] = lk[np.lexsort(lk.T[::-1])] if nl else lk
    if stepwise_tally:
        # the step-wise tally over the same cull: event count, tally flags and cull flags are fetched from the control block
        h.tally()
        t, g = h.get_tally()
        assert np.array_equal(t, s["tally"]) and np.array_equal(g, s["gaps"])
        pe2, ne2 = h.ins_events()
        assert ne2 == ne and np.array_equal(np.sort(hipapi.to_host(pe2, ne2, np.uint64)), s["events"])
    return s


def same(a, b, tag):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), (tag, k)


class Pair:
    """the default context and the one without the shadow launch, called side by side"""

    def __init__(self, w):
        self.w, self.hipapi = w, Hip()
        self.on, self.off = context(w, True), context(w, False)
        self.calls = 0

    def step(self, ref, circular=None):
        circular = self.w.circular if circular is None else circular
        self.calls += 1
        c_on, c_off = self.on.iterate(ref, circular), self.off.iterate(ref, circular)
        assert c_on == c_off, (self.calls, len(c_on), len(c_off))
        same(snapshot(self.on, self.hipapi, True), snapshot(self.off, self.hipapi, True), self.calls)
        return c_on

    def close(self):
        self.on.close()
        self.off.close()


def changed(s, at=None):
    at = len(s) // 3 if at is None else at
    return s[:at] + ("A" if s[at] != "A" else "C") + s[at + 1:]


def hit_miss_sequence(p, ref0):
    """ref0 -> c1 -> c2 -> c3 -> c4 (hits; the first call of a context whose reads carry inserts ends in the step-wise consensus, which
    enlarges the insert buffers; nothing adopts what was prepared behind it), c4 with one base changed (miss), ref0 again (miss), its result fed back (hit)"""
    c1 = p.step(ref0)
    assert c1 != ref0                      # (one column in a hundred of ref0 is not the reads')
    c2 = p.step(c1)
    c3 = p.step(p.step(c2))
    p.step(changed(c3, len(c3) - 1))       # the last byte
    p.step(changed(c3, 0))                 # ... and the first
    c5 = p.step(ref0)
    p.step(c5)


def against_the_oracle(oracle, w):
    import mia_amd
    from oracle_sample import check_subset_iterations
    done, _ = check_subset_iterations(mia_amd, oracle, w.ref0, w.circular, w.matrix_file, w.pssm, w.stored, w.rc, w.sk, w.as0, w.ae0, iters=3, lens=w.lens)
    assert done >= 2                       # (the second iteration is the first that adopts)


@pytest.mark.parametrize("matrix_file", [None, "ancient.submat.txt"], ids=["flat", "ancient"])
def test_circular_sequence(matrix_file, oracle):
    w = workload(11, 3000, 4000, True, matrix_file)
    against_the_oracle(oracle, w)
    p = Pair(w)
    hit_miss_sequence(p, w.ref0)
    p.close()


def test_linear_sequence(oracle):
    w = workload(12, 1500, 2000, False, "ancient.submat.txt")
    against_the_oracle(oracle, w)
    p = Pair(w)
    c1 = p.step(w.ref0)                    # (ends in the step-wise consensus: the reads carry inserts, the buffers are new)
    c2 = p.step(c1)
    c3 = p.step(c2)                        # hit
    p.step(changed(c3))
    p.step(p.step(w.ref0))                 # miss, hit
    p.close()


def test_length_change():
    """every read that covers column 700 carries two bases ref0 lacks: the consensus is two columns longer than its reference.  The shadow
    launch was queued for a string as long as the reference: its key is not the returned string's, it is dropped and the next call, whose
    wrapped stretch begins two columns later, prepares its own; the calls after that adopt"""
    w = workload(13, 2000, 3000, True, None, insertion_at=700)
    p = Pair(w)
    p.step(w.ref0)                         # (ends in the step-wise consensus, which enlarges the insert buffers)
    c1 = p.step(w.ref0)                    # the shadow launch read a string two columns longer than its key says: dropped
    assert len(c1) == len(w.ref0) + 2
    c2 = p.step(c1)                        # miss, on the longer string
    p.step(p.step(c2))                     # hits
    # back to the shorter string (the buffers do not shrink, their views must), and to the longer one
    p.step(w.ref0)
    p.step(c1)
    p.close()


def test_n_columns_in_the_consensus():
    """nobody covers columns 600 .. 619 of a linear reference: the consensus holds N there, the 10-mer table of the next call spells the
    10-mers around them out (kh_entries > 0, kwild > 0).  The shadow launch behind the first call was queued without any (kwild = 0) and read
    a string with N: its key is not the string's, so it is dropped; behind a reference with N none is queued"""
    w = workload(14, 1500, 2000, False, None, hole=(600, 620))
    p = Pair(w)
    c1 = p.step(w.ref0)
    assert "N" in c1[590:630]
    c2 = p.step(c1)
    p.step(c2)
    p.step(w.ref0)
    p.close()


def test_route_change_between_calls():
    """after the first hit the context gets another read set (another count: other grids and lists, and the plan's counters of the
    call before describe reads that are gone); the next call must be right whether it adopts or not"""
    w = workload(15, 1200, 3000, True, "ancient.submat.txt")
    p = Pair(w)
    c1 = p.step(w.ref0)
    c2 = p.step(c1)
    c3 = p.step(c2)                        # hit
    for h in (p.on, p.off):
        upload(h, w, 0, 2000)
    c4 = p.step(c3)
    p.step(c4)
    for h in (p.on, p.off):
        upload(h, w, 500, 3000)
        h.set_read_base(0)
    p.step(w.ref0)
    p.close()


def run_ranks(fns):
    out, err = [None] * len(fns), [None] * len(fns)

    def work(k):
        try:
            out[k] = fns[k]()
        except BaseException as e:        # noqa: BLE001 -- reported by the caller
            err[k] = e
    th = [threading.Thread(target=work, args=(k,)) for k in range(len(fns))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    return out, err


def test_two_rank_loopback():
    """two shards joined by the library's loopback transport, default build and switch-off build (each pair in its own build's group).  With a
    communicator nothing is prepared ahead: what is held here is that the doubled control block and the adoption test leave a sharded run
    as it was"""
    import mia_amd
    w = workload(16, 1500, 3000, True, None)
    hipapi = Hip()
    cut = 1301
    groups = []
    for ahead in (True, False):
        parts = [context(w, ahead, 0, cut), context(w, ahead, cut, w.n)]
        grp = mia_amd.LoopbackGroup(2, like=parts[0])
        for k, h in enumerate(parts):
            grp.attach(h, k)
        groups.append((parts, grp))
    ref = w.ref0
    for call, nxt in enumerate(["cons", "cons", "cons", "changed", "ref0", "cons"]):
        cons = []
        for parts, _ in groups:
            out, err = run_ranks([lambda h=h: h.iterate(ref, True) for h in parts])
            assert err == [None, None], (call, err)
            assert out[0] == out[1]
            cons.append(out[0])
        assert cons[0] == cons[1], call
        for k in range(2):
            # (no step-wise tally here: a rank's tally buffers hold the all-reduced words)
            same(snapshot(groups[0][0][k], hipapi, False), snapshot(groups[1][0][k], hipapi, False), (call, k))
        ref = {"cons": cons[0], "changed": changed(cons[0]), "ref0": w.ref0}[nxt]
    for parts, grp in groups:
        for h in parts:
            h.comm_destroy()
        grp.close()
        for h in parts:
            h.close()


CHILD = r"""
import os, sys
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "tools"), os.path.join(%(root)r, "tests")]
import test_gpu_ref_ahead as t
w = t.workload(17, 600, 2000, True, None, indel_rate=0.0)       # (no inserts: the first call does not end in the step-wise consensus)
h = t.context(w, True)
ref = w.ref0
for k, nxt in enumerate(["cons", "cons", "changed", "cons"]):
    sys.stderr.write("@@ call %%d\n" %% k); sys.stderr.flush()
    cons = h.iterate(ref, True)
    ref = cons if nxt == "cons" else t.changed(cons)
sys.stderr.write("@@ end\n")
h.close()
"""


def test_timing_lap_names_the_adoption():
    """MIA_HIP_TIMING=1 (release build): the host lap behind the reference stage reads `reference (ahead)` on a call that adopted --
    none on the first call, one on each fed-back call, none on the changed string"""
    env = dict(os.environ, MIA_HIP_TIMING="1")
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], env=env, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    calls = r.stderr.split("@@ call ")[1:]
    assert len(calls) == 4
    ahead = [c.count("reference (ahead)") for c in calls]
    plain = [sum(1 for line in c.split("\n") if "[mia_hip_iterate host] reference " in line and "(ahead)" not in line) for c in calls]
    assert ahead == [0, 1, 1, 0] and plain == [1, 0, 0, 1], (ahead, plain, r.stderr[-2000:])
