"""mia_hip_trim at its edges, on both of its GPU routes.

The lane kernel (k_trim) and the exact scalar kernel (k_trim_wide, a second implementation of the same DP with its own trace and
its own find_align_begin) are each held to the reference's own trim_frag on tests/golden/trim_vectors_edges.txt and
trim_vectors.txt: a context made under MIA_HIP_TRIM_EXACT=1 (alt build) re-runs EVERY read in k_trim_wide after k_trim has run.
Batches large enough that every wavefront of k_trim's persistent grid takes several reads, and that the exact re-run takes
several pieces, are compared read by read with the oracle's ora_trim (which test_oracle_vs_golden.py pins to the same vectors).
The functions that make the batches import no GPU code."""
import ctypes as C
import os
import random
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch      # (asked for the number of compute units; loaded here, before the library brings its HIP runtime into the process)

from test_oracle_vs_golden import trim_edge_vectors, trim_vectors

pytestmark = pytest.mark.gpu

NEAND = "GTCAGACACGCAACAGGGGATAGGCAAGGCACACAGGGGATAGG"
EXACT_PIECE = 4096       # TRIM_EXACT_PIECE of csrc/mia_trim_kernels.h: reads per k_trim_wide launch


def rseq(rnd, k, alphabet="ACGT"):
    return "".join(rnd.choices(alphabet, k=k))


def pack(reads):
    offs = np.zeros(len(reads) + 1, np.int64)
    offs[1:] = np.cumsum([len(r) for r in reads])
    return np.frombuffer("".join(reads).encode(), dtype=np.uint8), offs


def run_batch(hip, adapter, reads):
    bases, offs = pack(reads)
    trimmed, point = hip.trim(adapter, bases, offs)
    return [(int(t), int(p) if t else -999) for t, p in zip(trimmed, point)]


def oracle_trim(oracle, adapter, reads):
    """[(trimmed, trim_point or -999)] of ora_trim for every read, on eight host threads (ctypes calls release the interpreter lock)"""
    ad = adapter.encode()

    def part(lo):
        out = []
        tr, tp = C.c_int(), C.c_int()
        for r in reads[lo:lo + 512]:
            oracle.ora_trim(r.encode(), len(r), ad, C.byref(tr), C.byref(tp), None)
            out.append((tr.value, tp.value if tr.value else -999))
        return out

    with ThreadPoolExecutor(8) as ex:
        return [x for chunk in ex.map(part, range(0, len(reads), 512)) for x in chunk]


def assert_equal(got, want, reads, adapter):
    bad = [i for i in range(len(reads)) if got[i] != want[i]]
    assert not bad, (len(bad), adapter, [(i, reads[i], got[i], want[i]) for i in bad[:4]])


@pytest.fixture(scope="module")
def route():
    """route(name): the context of that name, made once -- "default", or "exact" (every read through k_trim_wide as well)"""
    import mia_amd
    made = {}

    def get(name):
        if name not in made:
            if name == "exact":
                os.environ["MIA_HIP_TRIM_EXACT"] = "1"
            try:
                made[name] = mia_amd.MiaHip(0)
            finally:
                os.environ.pop("MIA_HIP_TRIM_EXACT", None)
        return made[name]

    yield get
    for hip in made.values():
        hip.close()


def by_adapter(vectors):
    groups = {}
    for ad, read, exp in vectors:
        groups.setdefault(ad, []).append((read, tuple(exp[:2])))
    return groups


@pytest.mark.parametrize("which,name", [("edges", "default"), ("edges", "exact"), ("random", "exact")])
def test_reference_vectors_on_both_routes(route, which, name):
    """(trimmed, trim_point) of the reference's trim_frag for every vector, grouped by adapter: the edge vectors from k_trim with
    its escape re-runs and from k_trim_wide alone, the 500 random ones from k_trim_wide alone (test_gpu_trim.py has them on the
    default route)"""
    hip = route(name)
    vectors = [(ad, read, exp) for _, ad, read, exp in trim_edge_vectors()] if which == "edges" else trim_vectors()
    n = reruns = 0
    t0 = time.perf_counter()
    for ad, items in by_adapter(vectors).items():
        reads = [r for r, _ in items]
        got = run_batch(hip, ad, reads)
        assert_equal(got, [e for _, e in items], reads, ad)
        if name == "exact":
            assert hip.trim_exact_reruns() == len(items), ad
        reruns += hip.trim_exact_reruns()
        n += len(items)
    print(f"{which} vectors, {name} route: {n} reads, {reruns} exact re-runs, {time.perf_counter() - t0:.2f} s")
    assert n == len(vectors) and n >= (700 if which == "edges" else 500)
    if name == "default" and which == "edges":
        assert reruns >= 30       # the pairs built around 63+ unrelated bases


# ---- batches -----------------------------------------------------------------------------------------------------------------
def adapter_127():
    return rseq(random.Random(127), 127, "ACG")      # (no T: an all-T read body then gives the fresh-start reads their abr > 0)


def mixed_reads(adapter, n, seed):
    """n reads for one adapter, kinds shuffled by the seed: a fifth of at most 8 bases; a tenth adapter prefix + 63 .. 75
    unrelated bases + rest of the adapter (on the best path only where the adapter is long enough: 200 * len(adapter) -
    (1000 + 200 * 63) has to beat row 0's -600, so never with 44 bases); fresh starts (all-T body, read ends in
    adapter[a0 : a0 + m]); N; and bodies of every length with none, part or all of the adapter behind them"""
    rnd = random.Random(seed)
    la = len(adapter)
    reads = []
    for _ in range(n):
        u = rnd.random()
        if u < 0.2:
            k = rnd.randint(1, 8)
            r = rseq(rnd, k) if rnd.random() < 0.5 else (rseq(rnd, k) + adapter[: rnd.randint(1, la)])[-k:]
        elif u < 0.3 and la > 40:
            k = rnd.randint(33, min(50, la - 4))
            r = rseq(rnd, rnd.randint(0, 20)) + adapter[:k] + rseq(rnd, rnd.randint(63, 75)) + adapter[k:]
        elif u < 0.45 and la > 1:
            a0 = rnd.randint(1, min(30, la - 1))
            m = rnd.randint(min(6, la - a0), min(la - a0, a0 + 15))
            r = "T" * rnd.randint(1, 120) + adapter[a0:a0 + m]
        elif u < 0.6:
            lst = list(rseq(rnd, rnd.randint(1, 200)) + adapter[: rnd.randint(0, la)])
            for _ in range(rnd.randint(1, 4)):
                lst[rnd.randrange(len(lst))] = "N"
            r = "".join(lst)
        else:
            ln = rnd.randint(1, 256)
            tail = adapter[: rnd.choice([0, 0, rnd.randint(1, la), la])][:ln]
            r = rseq(rnd, ln - len(tail)) + tail
        reads.append(r[:256])
    return reads


def test_mixed_batch_every_wavefront_takes_three_reads(route, oracle):
    """3 * 32 * compute units + 17 reads per call, so that every wavefront of k_trim's persistent grid (at most 32 per compute
    unit) takes at least three: a wavefront's LDS sub-table, trace slab and column scratch pass from long reads to short ones,
    and ordinary reads follow escaping ones.  Three adapters (44, 1 and 127 bases) in three calls on ONE context; every read
    against ora_trim.  Re-runs: the 44-base adapter cannot have any (mixed_reads) and must show none, so the 300 are asked of
    the 127-base one."""
    hip = route("default")
    n = 3 * 32 * torch.cuda.get_device_properties(0).multi_processor_count + 17
    reruns = {}
    t_gpu = t_ora = 0.0
    for k, adapter in enumerate((NEAND, "G", adapter_127())):
        reads = mixed_reads(adapter, n, 1000 + k)
        t0 = time.perf_counter()
        got = run_batch(hip, adapter, reads)
        t1 = time.perf_counter()
        want = oracle_trim(oracle, adapter, reads)
        t_gpu, t_ora = t_gpu + t1 - t0, t_ora + time.perf_counter() - t1
        reruns[len(adapter)] = hip.trim_exact_reruns()
        assert_equal(got, want, reads, adapter)
        lens = [len(r) for r in reads]
        assert sum(t for t, _ in want) >= 1000 and sum(1 - t for t, _ in want) >= 1000, adapter
        assert sum(1 for x in lens if x <= 8) >= n // 6 and min(lens) == 1 and max(lens) == 256
    print(f"mixed batch: 3 x {n} reads, exact re-runs by adapter length {reruns}, GPU calls {t_gpu:.2f} s, oracle {t_ora:.2f} s")
    assert reruns[127] >= 300 and reruns[44] == 0 and reruns[1] == 0, reruns


def test_exact_rerun_in_pieces(route, oracle):
    """2.5 pieces' worth of reads in one call under MIA_HIP_TRIM_EXACT=1, 127-base adapter: two full launches of k_trim_wide and
    a partial one on ONE scratch of one piece's size (0.55 GB, below the 1 GiB the re-run may take however many reads need it:
    one allocation for all 10 240 reads would be 1.4 GB), equal to ora_trim read by read; then a small call on the same
    context, whose scratch is its seven reads' worth"""
    hip = route("exact")
    adapter = adapter_127()
    n = 2 * EXACT_PIECE + EXACT_PIECE // 2
    reads = mixed_reads(adapter, n, 77)
    t0 = time.perf_counter()
    got = run_batch(hip, adapter, reads)
    dt = time.perf_counter() - t0
    assert hip.trim_exact_reruns() == n
    per_read = (len(adapter) * 256 + 5 * 256) * 4
    launches, scratch = hip.trim_rerun_stats()
    print(f"exact re-run of {n} reads in pieces of {EXACT_PIECE}: {dt:.2f} s, {launches} launches, scratch {scratch} bytes")
    assert launches == 3 and scratch == EXACT_PIECE * per_read and scratch <= 2 ** 30 < n * per_read
    assert_equal(got, oracle_trim(oracle, adapter, reads), reads, adapter)
    few = reads[EXACT_PIECE - 3:EXACT_PIECE + 4]
    assert run_batch(hip, adapter, few) == got[EXACT_PIECE - 3:EXACT_PIECE + 4]
    assert hip.trim_exact_reruns() == len(few) and hip.trim_rerun_stats() == (1, len(few) * per_read)


# ---- call edges --------------------------------------------------------------------------------------------------------------
def test_call_edges(route, oracle):
    import mia_amd
    hip = route("default")
    adapter = adapter_127()
    reads = mixed_reads(adapter, 300, 5)
    bases, offs = pack(reads)
    whole = hip.trim(adapter, bases, offs)
    assert hip.trim_exact_reruns() > 0
    assert [(int(t), int(p) if t else -999) for t, p in zip(*whole)] == oracle_trim(oracle, adapter, reads)
    # offsets[0] != 0: a slice of the larger buffer answers as the slice alone does
    part = hip.trim(adapter, bases, offs[100:221])
    assert np.array_equal(part[0], whole[0][100:220]) and np.array_equal(part[1], whole[1][100:220])
    alone = hip.trim(adapter, *pack(reads[100:220]))
    assert np.array_equal(part[0], alone[0]) and np.array_equal(part[1], alone[1])
    # n = 1
    one = hip.trim(adapter, bases, offs[7:9])
    assert (int(one[0][0]), int(one[1][0])) == (int(whole[0][7]), int(whole[1][7]))
    # n = 0 after a call that had re-runs: the count is that of the most recent call
    hip.trim(adapter, bases, offs)
    assert hip.trim_exact_reruns() > 0
    t, p = hip.trim(adapter, np.zeros(0, np.uint8), np.zeros(1, np.int64))
    assert len(t) == 0 and len(p) == 0 and hip.trim_exact_reruns() == 0 and hip.trim_rerun_stats() == (0, 0)
    # refused arguments: MIA_HIP_ERR_ARG (-2), and the context goes on working
    b3, o3 = pack(["ACG", "ACGT", "A"])
    for ad, b, o in (("", b3, o3), ("A" * 128, b3, o3), ("ACGT", b3, np.array([0, 3, 3, 8], np.int64)),
                     ("ACGT", *pack(["ACG", "A" * 257]))):
        with pytest.raises(mia_amd.MiaHipError, match=r"error -2\b"):
            hip.trim(ad, b, o)
        again = hip.trim(adapter, bases, offs[7:9])
        assert (int(again[0][0]), int(again[1][0])) == (int(whole[0][7]), int(whole[1][7]))
