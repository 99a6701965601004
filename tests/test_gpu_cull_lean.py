"""k_cull_records' lean form (an iteration of mia_hip_iterate without a link leaves the slot numbers and the link side arrays unwritten)
and its one-round-trip loads, held against the same library with the lean form switched off (MIA_HIP_NO_CULL_LEAN) and with the
tally records written by k_rec_params in every iteration (MIA_HIP_NO_CULL_RECORDS): three contexts side by side, three calls of
iterate each, and after every call record_params(), dropped(), alignments(), get_tally(), the consensus and the links (as a sorted
set: they are appended with atomics) must be equal.

Per shape three runs: links planted before the first call (set_back_slots: a non-split read whose back pointer names a live slot,
kind 0; set_pass1_state: strand-unknown reads with pass-1 slots, kinds 1 and 2; both on the first and the last read of a block), no
link at all, and links planted and taken away between the calls (lean, full, lean in one context).  mia_hip_cull_stats must report
the number of links before the cull ran, and the lean form exactly in the calls that emitted none.

Shapes: 100-base reads of both strands on a 700 bp circular reference (about one read in seven runs over the origin: two records)
and on a 40 kb linear one (313 tally buckets); n at every edge of a wavefront, a block of 256 and a group of sixteen blocks."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NS = [1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 3 * 4096 + 17]
REFS = {"circ700": (700, True), "lin40k": (40_000, False)}
ENVS = [None, "MIA_HIP_NO_CULL_LEAN", "MIA_HIP_NO_CULL_RECORDS"]
MID = 300                       # a start in the middle of either reference: such a read is not split


class Hip:
    """hipMemcpy through ctypes: the links are handed out as a device pointer"""

    def __init__(self):
        self.l = C.CDLL("libamdhip64.so")
        self.l.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]

    def to_host(self, dptr, n, dtype):
        out = np.empty(n, dtype)
        if n:
            assert self.l.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(dptr), out.nbytes, 2) == 0
        return out


_WORKLOADS = {}


def plant(n):
    """(reads of kind 0, strand-unknown reads) for n reads: distinct, block edges included where n has them"""
    kind0 = [i for i in (2, 255, n - 1) if 0 <= i < n]
    unknown = [i for i in (0, 5, 256, 511) if i < n and i not in kind0 and n >= 8]
    return sorted(set(kind0)), unknown


def workload(ref_name, n):
    """computed once per shape and not changed by the tests"""
    key = (ref_name, n)
    if key not in _WORKLOADS:
        import gen_data
        import mia_amd
        L, circular = REFS[ref_name]
        ref = gen_data.random_reference(L, seed=L)
        rng = np.random.default_rng(n + L)
        start = rng.integers(0, L if circular else L - 108, n)
        kind0, unknown = plant(n)
        start[kind0 + unknown] = MID
        d = gen_data.make_reads(ref, n, 100, seed=n + 1, circular=circular, start=start)
        w = {"ref": ref, "circular": circular, "n": n, "pssm": mia_amd.flat_pssm(), "stored": gen_data.stored_orientation(d).reshape(-1),
             "offsets": np.arange(n + 1, dtype=np.int64) * 100, "rc": d["strand"].astype(np.uint8), "as_": start.astype(np.int32),
             "ae": (start + 99).astype(np.int32), "kind0": kind0, "unknown": unknown}
        for v in w.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _WORKLOADS[key] = w
    return _WORKLOADS[key]


def planted_pointers(w, with_unknown):
    """back_slot, front_slot0: every pointer names a slot of its own among the first records of the iteration (live: there are at
    least as many records as strand-known reads)"""
    n = w["n"]
    back, front = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    t = 0
    for i in w["kind0"]:
        back[i] = t
        t += 1
    if with_unknown:
        for k, i in enumerate(w["unknown"]):
            front[i] = t
            t += 1
            if k != 1:                        # (the second one keeps a front pointer only)
                back[i] = t
                t += 1
    assert t <= n - (len(w["unknown"]) if with_unknown else 0)
    return back, front


def context(w, env, sk):
    import mia_amd
    if env:
        os.environ[env] = "1"
    try:
        h = mia_amd.MiaHip(0)
    finally:
        if env:
            os.environ.pop(env, None)
    assert h.is_alt_build == (env is not None)
    h.set_pssm(w["pssm"])
    h.upload_reads(w["stored"], w["offsets"], w["rc"], sk, w["as_"], w["ae"])
    return h


def snapshot(h, hipapi, cons):
    s = {"cons": np.frombuffer(cons.encode(), np.uint8)}
    s["score"], s["as"], s["ae"] = h.alignments()
    s["dropped_f"], s["dropped_b"] = h.dropped()
    s["params"], s["back_slot"] = h.record_params()
    s["tally"], s["gaps"] = h.get_tally()
    pl, nl = h.links()
    lk = hipapi.to_host(pl, 4 * nl, np.int64).reshape(-1, 4)
    s["links"] = lk[np.lexsort(lk.T[::-1])] if nl else lk
    return s


def three_calls(w, scenario):
    """-> [(links of the call, lean as the default context reports it)] of the three calls; everything else is asserted here"""
    n, hipapi = w["n"], Hip()
    sk = np.ones(n, np.uint8)
    if scenario == "planted":
        sk[w["unknown"]] = 0
    hs = [context(w, env, sk) for env in ENVS]
    try:
        if scenario == "planted":
            back, front = planted_pointers(w, True)
            score = np.where(sk == 0, 2000, 0).astype(np.int32)       # a strand-unknown read keeps its pass-1 score: exactly the cutoff
            for h in hs:
                h.set_pass1_state(front, back, score)
        refs, calls = [w["ref"]] * 3, []
        for call in range(3):
            if scenario == "between" and call in (1, 2):
                # call 1 with the planted back pointers beside the ones the split reads hold by now, call 2 with none at all
                back = planted_pointers(w, False)[0] if call == 1 else np.full(n, -1, np.int64)
                for h in hs:
                    cur = h.record_params()[1]
                    h.set_back_slots(np.where(back >= 0, back, cur) if call == 1 else back)
            snaps, stats = [], []
            for k, h in enumerate(hs):
                cons = h.iterate(refs[k], w["circular"])
                refs[k] = cons
                snaps.append(snapshot(h, hipapi, cons))
                stats.append(h.cull_stats())
            for k in (1, 2):
                assert sorted(snaps[0]) == sorted(snaps[k])
                for name in snaps[0]:
                    assert snaps[0][name].shape == snaps[k][name].shape and np.array_equal(snaps[0][name], snaps[k][name]), (scenario, call, ENVS[k], name)
            n_links = len(snaps[0]["links"])
            print("%s call %d: %d links, stats %s" % (scenario, call, n_links, stats))
            # the count taken before the cull is the number of links it emitted; lean exactly without a link, and only by default
            assert [s[0] for s in stats] == [n_links] * 3
            assert [s[1] for s in stats] == [n_links == 0, False, False]
            calls.append((n_links, stats[0][1]))
        return calls
    finally:
        for h in hs:
            h.close()


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("ref_name", sorted(REFS))
def test_lean_and_full_culls_give_the_same_iterations(ref_name, n):
    w = workload(ref_name, n)
    planted = three_calls(w, "planted")
    none = three_calls(w, "none")
    between = three_calls(w, "between")
    # conditions on the inputs: every shape sees a call of each kind, and the planted pointers all became links
    want = len(w["kind0"]) + sum(1 if k == 1 else 2 for k in range(len(w["unknown"])))
    assert all(c[0] >= want and not c[1] for c in planted)
    assert any(c[1] for c in none)
    assert between[0][1] and between[1][0] >= len(w["kind0"]) and not between[1][1] and between[2][1]


def test_step_wise_link_calls_are_refused_after_a_lean_cull():
    import mia_amd
    w = workload("circ700", 257)
    sk = np.ones(w["n"], np.uint8)
    lean, full = context(w, None, sk), context(w, "MIA_HIP_NO_CULL_LEAN", sk)
    try:
        for h in (lean, full):
            h.iterate(w["ref"], w["circular"])
        assert lean.cull_stats() == (0, True) and full.cull_stats() == (0, False)
        ptr, cnt = lean.links()
        for call in (lambda: lean.set_links(ptr, cnt), lean.link_lengths, lean.finish_links):
            with pytest.raises(mia_amd.MiaHipError, match="mia_hip_cull first"):
                call()
        full.link_lengths()
        full.finish_links()
        # a step-wise cull writes everything again: the calls go through and both contexts hold the same records
        for h in (lean, full):
            h.cull(hard_cut=2500)
            assert h.cull_stats() == (0, False)
            h.link_lengths()
            h.finish_links()
        a, b = lean.record_params(), full.record_params()
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        for x, y in zip(lean.dropped(), full.dropped()):
            assert np.array_equal(x, y)
    finally:
        lean.close()
        full.close()
