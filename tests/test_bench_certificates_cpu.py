"""No GPU: tests/golden/bench_certificates.json -- written by the HIP path (tools/make_bench_certificates.py), what bench.py's
line must show -- against tests/golden/bench_certificates_ref.json -- written from the REFERENCE's own loop on every read of
the same workloads (tools/make_ref_certificates.py, oracle/_ref/ref_iter_driver).  All pinned runs converge in two iterations, so
the HIP certificate's final step is the reference's iteration 2."""
import json
import os

import pytest

import ref_certificates as rc
from conftest import GOLDEN

HIP = json.load(open(os.path.join(GOLDEN, "bench_certificates.json")))
REF = rc.load()
SIZES = {"cfg1": 1_000_000, "cfg2": 1_000_000, "cfg3": 10_000_000}


def is_hex(s, n):
    return len(s) == n and all(c in "0123456789abcdef" for c in s)


@pytest.mark.parametrize("key", sorted(SIZES))
def test_hip_certificate_is_the_references(key):
    hip, ref = HIP[key], REF[key]
    assert hip["workload"] == ref["workload"]
    assert hip["iterations_to_convergence"] == 2 and hip["consensus_is_fixed_point"]
    assert (hip["consensus_sha256"], hip["consensus_len"]) == (ref["consensus_sha256"], ref["consensus_len"])
    assert hip["alignments_sha256"] == ref["iterations"]["2"]["alignments_sha256"]


@pytest.mark.parametrize("key", sorted(SIZES))
def test_reference_golden_schema(key):
    e = REF[key]
    assert e["reads"] == SIZES[key] and e["block"] == REF["block"] == 8192
    assert e["made_by"] == "oracle/_ref/ref_iter_driver" and 0 < e["chunk"] <= 50_000
    assert sorted(e["iterations"]) == ["1", "2"]
    for it in e["iterations"].values():
        assert is_hex(it["alignments_sha256"], 64)
        assert len(it["blocks"]) == -(-e["reads"] // 8192) and all(is_hex(b, 16) for b in it["blocks"])
    assert e["iterations"]["1"]["alignments_sha256"] != e["iterations"]["2"]["alignments_sha256"]


@pytest.mark.parametrize("cfg", [1, 2])
def test_prefix_entries(cfg):
    p, whole = REF["cfg%d_prefix" % cfg], REF["cfg%d" % cfg]
    assert p["reads"] == 200_000 and p["made_by"] == "oracle/_ref/ref_iter_driver"
    assert p["workload"] == whole["workload"] + "[:200000]"
    assert p["iterations_run"] in (2, 3) and sorted(p["iterations"]) == [str(k) for k in range(1, p["iterations_run"] + 1)]
    last, before = p["iterations"][str(p["iterations_run"])], p["iterations"][str(p["iterations_run"] - 1)]
    assert last["consensus_sha256"] == before["consensus_sha256"]                  # run to the fixed point
    for it in p["iterations"].values():
        assert is_hex(it["consensus_sha256"], 64) and is_hex(it["alignments_sha256"], 64) and it["consensus_len"] > 0
        assert len(it["blocks"]) == -(-200_000 // 8192)
    # chunk independence, as far as digests can show it: 24 whole blocks of the prefix are blocks of the chunked run
    for k in ("1", "2"):
        assert p["iterations"][k]["blocks"][:24] == whole["iterations"][k]["blocks"][:24]


def test_chunk_independence_and_the_gap_are_written_down():
    assert REF["chunk_independent"] is True
    assert REF["made_by"] == "oracle/_ref/ref_iter_driver"
    assert set(REF["cfg4"]) == {"not_covered"} and len(REF["cfg4"]["not_covered"]) > 40
    assert os.path.getsize(rc.REF_FILE) < 1_000_000
