"""A pass 1 in the middle of a job.  The anchored stage of mia_hip_pass1 lends the context to align_all (AlignBorrow, csrc/mia_hip_tools.inc)
and must put it back: the job's later steps give what they give without the pass 1, and the stage timers and read counters of the
iteration path do not see the borrowed run.  The second test pins pass 1's refusals, code and message, none of which runs a kernel."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from mia_flow import fsdb_arrays, hip_iteration, oracle_after_pass1, pssm_array
from test_gpu_pass1 import read_fasta, ref_fasta

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -2, -4


def start_job(oracle):
    """golden tr1.fna / tf.fna with the flat matrix on a new context, as test_gpu_context_reuse.py uploads it"""
    st, _opts, anc = oracle_after_pass1(oracle, "tr1.fna", "tf.fna", True, -1, None)
    fs = fsdb_arrays(oracle, st)
    ref = oracle.ora_ref_seq(st)[:oracle.ora_ref_len(st)].decode()
    dropped = np.array([oracle.ora_slot_at(st, i).contents.dropped for i in range(oracle.ora_num_culled(st))], np.uint8)
    oracle.ora_free(st)
    import mia_amd
    hip = mia_amd.MiaHip(0)
    hip.set_pssm(pssm_array(anc))
    hip.upload_reads(fs["bases"], fs["offsets"], fs["rc"], fs["sk"], fs["as_"], fs["ae"])
    hip.set_slot_dropped(dropped)
    hip.set_pass1_state(fs["front"], fs["back"], fs["score"])
    return hip, fs, ref


def step(hip, fs, ref, fused):
    lens = (fs["offsets"][1:] - fs["offsets"][:-1]).astype(np.int32)
    sk = fs["sk"].astype(bool)
    score, as_, ae, cons = hip_iteration(hip, ref, True, lens, fused=fused)
    cols, rstart = hip.scripts()
    dF, dB = hip.dropped()
    prm, back = hip.record_params()
    # (a read of unknown strand is never re-aligned and has no script; rows past a read's length belong to nobody)
    return dict(cons=cons, score=score, as_=as_, ae=ae, rstart=rstart[sk], dF=dF, dB=dB, prm=prm, back=back,
                rows=[cols[i, :lens[i]].copy() for i in np.flatnonzero(sk)])


def counters(hip):
    """what the iteration path's statistics calls report; bx_stats' launch count is left out (a borrowed run adds to it)"""
    stages = {k: v for k, v in hip.stage_stats().items() if k != "k_pass1"}
    return dict(stages=stages, bx_reads=hip.bx_stats()[0], filter=hip.filter_stats(), plain=hip.plain_stats())


def s150():
    reads = [s for _, s in read_fasta(os.path.join(GOLDEN, "s150.fa")) if len(s) > 0]
    offsets = np.zeros(len(reads) + 1, np.int64)
    offsets[1:] = np.cumsum([len(s) for s in reads])
    return np.frombuffer("".join(reads).encode(), dtype=np.uint8), offsets


FUSED = (True, True, False)


def test_a_pass1_between_two_steps_leaves_the_job_alone(oracle):
    a, fs, ref = start_job(oracle)
    want = []
    for fused in FUSED:
        want.append(step(a, fs, ref, fused))
        ref = want[-1]["cons"]
    a.close()
    assert len(want[0]["cons"]) > 0

    b, fs, ref = start_job(oracle)
    got = [step(b, fs, ref, FUSED[0])]
    bases, offsets = s150()
    assert len(offsets) - 1 == 150
    before = counters(b)
    # 150 reads against a reference full of N: the filter is off, the anchored windows (and with them the borrowed align_all) take them
    b.pass1(ref_fasta(os.path.join(GOLDEN, "mt311.fa")), True, bases, offsets, -1)
    after = counters(b)
    assert b.pass1_filtered() == 0 and b.pass1_anchored() > 0
    assert sum(k for _, k in before["stages"].values()) > 0      # (the first step's launches are in the timers the call must not touch)
    assert after == before
    for fused in FUSED[1:]:
        got.append(step(b, fs, got[-1]["cons"], fused))
    b.close()
    for k in (0, 1, 2):
        g, w = got[k], want[k]
        assert g["cons"] == w["cons"], k
        for f in ("score", "as_", "ae", "rstart", "dF", "dB", "prm", "back"):
            assert np.array_equal(g[f], w[f]), (k, f)
        assert len(g["rows"]) == len(w["rows"])
        for i, (x, y) in enumerate(zip(g["rows"], w["rows"])):
            assert np.array_equal(x, y), (k, "script of known-strand read", i)


def test_refusals_name_their_cause_and_run_nothing():
    import mia_amd
    ref = "ACGTTGCA" * 40
    hip = mia_amd.MiaHip(0)

    def refused(code, message, bases, offsets, kmer=-1):
        with pytest.raises(mia_amd.MiaHipError) as e:
            hip.pass1(ref, True, np.frombuffer(bases.encode(), np.uint8), np.asarray(offsets, np.int64), kmer)
        assert str(e.value) == "libmia_hip error %d: %s" % (code, message)

    one = ("ACGT" * 10, [0, 40])
    refused(ERR_STATE, "set_pssm must precede pass1", *one)
    hip.set_pssm(mia_amd.flat_pssm())
    refused(ERR_ARG, "Cannot use kmer length greater than 14", *one, kmer=15)
    refused(ERR_ARG, "read length outside 1..256", "ACGT" * 10, [0, 40, 40])                  # a read of length 0
    refused(ERR_ARG, "read length outside 1..256", "A" * 297, [0, 40, 297])                   # ... and one of 257
    out = hip.pass1(ref, True, np.zeros(0, np.uint8), np.zeros(1, np.int64), -1)              # no reads: nothing to do, no error
    assert all(len(x) == 0 for x in out)
    hip.close()
