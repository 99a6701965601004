"""Test plumbing: every read of a benched workload against tests/golden/bench_certificates_ref.json, the digests of what the
REFERENCE's own loop computes for them (oracle/_ref/ref_iter_driver, tools/make_ref_certificates.py) -- unlike
bench_certificates.json, which the HIP path wrote itself.  A whole-array mismatch is narrowed to the first block of 8 192 reads
whose digest differs, and that block is run through the oracle to name the reads.  TEST INFRASTRUCTURE."""
import hashlib
import json
import os

import numpy as np

from conftest import GOLDEN

REF_FILE = os.path.join(GOLDEN, "bench_certificates_ref.json")


def load(path=REF_FILE):
    with open(path) as f:
        return json.load(f)


def digest(score, as_, ae):
    """bench.certificate's layout: int32 little endian, the three arrays one after the other"""
    h = hashlib.sha256()
    for x in (score, as_, ae):
        h.update(np.ascontiguousarray(x, dtype="<i4").tobytes())
    return h.hexdigest()


def consensus_digest(cons):
    return hashlib.sha256(cons.encode()).hexdigest()


def bad_blocks(al, want, block):
    """indices of the blocks of `block` reads whose 16-hex digest is not the golden's"""
    n = len(al[0])
    assert len(want) == -(-n // block), (len(want), n, block)
    return [b for b in range(len(want)) if digest(*(x[b * block:(b + 1) * block] for x in al))[:16] != want[b]]


def oracle_rerun(oracle, refs, circular, matrix_file, stored, rc, as0, ae0):
    """-> f(lo, hi): the oracle's (score, as, ae) of reads [lo, hi) after iterating them alone through `refs` from (as0, ae0)"""
    from oracle_sample import PushedOracle

    def run(lo, hi):
        po = PushedOracle(oracle, refs[0], circular, matrix_file, stored[lo:hi], rc[lo:hi], as0[lo:hi], ae0[lo:hi])
        for ref in refs:
            po.iterate(ref)
        out = tuple(x.copy() for x in po.alignments())
        po.close()
        return out
    return run


def check_alignments(al, entry, it, what, rerun=None):
    """al = (score, as, ae) of every read after iteration `it`; entry = the golden's record of that workload.
    rerun: oracle_rerun(...) for this iteration, used only to turn a mismatch into read indices."""
    want = entry["iterations"][str(it)]
    n = len(al[0])
    assert n == entry["reads"], (what, n, entry["reads"])
    got = digest(*al)
    if got == want["alignments_sha256"]:
        return
    block = entry.get("block", 8192)
    bad = bad_blocks(al, want["blocks"], block)
    msg = "%s iteration %d: alignments %s, the reference's %s; %d of %d blocks of %d reads differ, first %s" % (
        what, it, got[:16], want["alignments_sha256"][:16], len(bad), len(want["blocks"]), block, bad[:8])
    if bad and rerun is not None:
        lo, hi = bad[0] * block, min((bad[0] + 1) * block, n)
        o = rerun(lo, hi)
        diff = np.nonzero((al[0][lo:hi] != o[0]) | (al[1][lo:hi] != o[1]) | (al[2][lo:hi] != o[2]))[0]
        if len(diff):
            show = [(int(lo + i), tuple(int(x[lo + i]) for x in al), tuple(int(x[i]) for x in o)) for i in diff[:8]]
            msg += "; block %d = reads [%d, %d): %d reads differ from the oracle, (read, hip, oracle): %s" % (bad[0], lo, hi, len(diff), show)
        else:
            msg += ("; block %d = reads [%d, %d): the ORACLE agrees with HIP on all of them while the reference's digest does not -- "
                    "the oracle has drifted from the reference (fix oracle/, pin the reads under tests/golden/)" % (bad[0], lo, hi))
    raise AssertionError(msg)


def check_consensus(cons, sha, length, what):
    assert (consensus_digest(cons), len(cons)) == (sha, length), (what, consensus_digest(cons)[:16], len(cons), sha[:16], length)
