"""One context, three jobs: a small one, a larger one (more reads, a longer reference, a position-specific matrix: every buffer of the
context grows), the small one again (fewer reads and a shorter reference under capacities that are now larger).  Whatever a job
leaves in the context -- a kernel's view of a block that growth has freed, a capacity that no longer belongs to its block -- shows
as a difference from what a FRESH context gives for the same job (those results are pinned to the oracle by
test_gpu_iteration.py::test_iterations_match_oracle).  Then the context is closed and another one made in the same process."""
import numpy as np
import pytest

from mia_flow import fsdb_arrays, hip_iteration, oracle_after_pass1, pssm_array

pytestmark = pytest.mark.gpu

# (ref, reads, pssm file, k-mer length of pass 1): all circular
SMALL = ("tr1.fna", "tf.fna", None, -1)
LARGE = ("mt311.fa", "s150.fa", "ancient.submat.txt", 12)


def job_inputs(oracle, job):
    ref_fa, reads_fa, pfile, kmer = job
    st, _opts, anc = oracle_after_pass1(oracle, ref_fa, reads_fa, True, kmer, pfile)
    fs = fsdb_arrays(oracle, st)
    L0 = oracle.ora_ref_len(st)
    inp = dict(fs=fs, pssm=pssm_array(anc), ref=oracle.ora_ref_seq(st)[:L0].decode(),
               slot_dropped=np.array([oracle.ora_slot_at(st, i).contents.dropped for i in range(oracle.ora_num_culled(st))], np.uint8),
               lens=(fs["offsets"][1:] - fs["offsets"][:-1]).astype(np.int32))
    oracle.ora_free(st)
    return inp


def run_job(hip, inp):
    """the job on `hip`: two mia_hip_iterate steps, then one iteration through realign / cull / tally / consensus; what each left behind"""
    fs = inp["fs"]
    hip.set_pssm(inp["pssm"])
    hip.upload_reads(fs["bases"], fs["offsets"], fs["rc"], fs["sk"], fs["as_"], fs["ae"])
    hip.set_slot_dropped(inp["slot_dropped"])
    hip.set_pass1_state(fs["front"], fs["back"], fs["score"])
    sk = fs["sk"].astype(bool)
    ref, steps = inp["ref"], []
    for fused in (True, True, False):
        score, as_, ae, cons = hip_iteration(hip, ref, True, inp["lens"], fused=fused)
        cols, rstart = hip.scripts()
        # (a read of unknown strand is never re-aligned and has no script; rows past a read's length belong to nobody)
        rows = [cols[i, :inp["lens"][i]].copy() for i in np.flatnonzero(sk)]
        dF, dB = hip.dropped()
        prm, back = hip.record_params()
        steps.append(dict(score=score, as_=as_, ae=ae, rows=rows, rstart=rstart[sk], dF=dF, dB=dB, prm=prm, back=back, cons=cons))
        ref = cons
    return steps


def assert_same(got, want, what):
    assert len(got) == len(want) == 3
    for k, (g, w) in enumerate(zip(got, want)):
        assert g["cons"] == w["cons"], (what, k)
        for f in ("score", "as_", "ae", "rstart", "dF", "dB", "prm", "back"):
            assert np.array_equal(g[f], w[f]), (what, k, f)
        assert len(g["rows"]) == len(w["rows"])
        for i, (a, b) in enumerate(zip(g["rows"], w["rows"])):
            assert np.array_equal(a, b), (what, k, "script of known-strand read", i)


def test_a_context_gives_every_job_what_a_fresh_one_gives(oracle):
    import mia_amd
    small, large = job_inputs(oracle, SMALL), job_inputs(oracle, LARGE)
    assert large["fs"]["n"] > small["fs"]["n"] and len(large["ref"]) > len(small["ref"])      # the second job makes everything grow
    fresh = {}
    for name, inp in (("small", small), ("large", large)):
        hip = mia_amd.MiaHip(0)
        fresh[name] = run_job(hip, inp)
        hip.close()
    assert len(fresh["small"][0]["cons"]) > 0 and len(fresh["large"][0]["cons"]) > 0
    hip = mia_amd.MiaHip(0)
    for leg, (name, inp) in enumerate((("small", small), ("large", large), ("small", small))):
        assert_same(run_job(hip, inp), fresh[name], "leg %d (%s)" % (leg + 1, name))
    hip.close()
    # ... and a context made after another was destroyed in this process
    again = mia_amd.MiaHip(0)
    assert_same(run_job(again, small), fresh["small"], "second context")
    again.close()
