"""The ACE export (ma -f 7) and the rewrite (ma -m) without a GPU.  tests/ma_ace_ref.py restates ace_output and write_ma in Python; it must
reproduce every output recorded from the reference's own `ma` (tests/golden/ma_ace, written by tools/make_ma_ace_goldens.py from
oracle/_ref/ma) byte for byte -- the ACE text from its first line, the rewritten file from its second.  The code the ACE kernels run per
record (csrc/ma_ace_body.h) and ma_hip's reader and writer (host/maln_text.h) are compiled for the host into tests/ma_ace_driver.cpp,
with -fsanitize=address,undefined where g++ has that runtime, and must agree with the restatement on every record and every file."""
import gzip
import hashlib
import json
import os
import re
import subprocess

import pytest

import ma_ace_ref as ref
import maln_ace_cases as mc
import maln_synth as ms
from conftest import GOLDEN, ROOT

ACE = os.path.join(GOLDEN, "ma_ace")


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(ACE, "runs.json")) as f:
        runs = json.load(f)
    with open(os.path.join(ACE, "hashes.json")) as f:
        hashes = json.load(f)
    with gzip.open(os.path.join(ACE, "outputs.json.gz")) as f:
        outputs = json.load(f)
    return runs, hashes, outputs


@pytest.fixture(scope="module")
def cases():
    return {name: mc.make_case(name) for name in mc.CASES + mc.SCAN_EDGES}


def sanitizer_flags(tmp):
    """-fsanitize=address,undefined if a program built with it links and runs here"""
    src, exe = tmp / "probe.cpp", tmp / "probe"
    src.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    ok = subprocess.run(["g++"] + flags + ["-o", str(exe), str(src)], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode == 0
    return flags if ok and subprocess.run([str(exe)]).returncode == 0 else []


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ma_ace")
    flags = sanitizer_flags(tmp)
    print("ma_ace_driver: sanitizers", "on" if flags else "not available: compiled without")
    exe = tmp / "ma_ace_driver"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-g"] + flags + ["-o", str(exe), os.path.join(ROOT, "tests", "ma_ace_driver.cpp")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()
    return str(exe)


def check(recorded, name, key, what, data):
    _, hashes, outputs = recorded
    h = hashes[f"{name}.{key}.{what}"]
    full = outputs[name][key].get(what)
    raw = data.encode("latin1")
    if full is not None and raw != full.encode("latin1"):
        a, b = data.split("\n"), full.split("\n")
        at = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        pytest.fail(f"{name} {key} {what}: line {at + 1}: {a[at:at + 1]!r} instead of {b[at:at + 1]!r}")
    assert (len(raw), hashlib.sha256(raw).hexdigest()) == (h["bytes"], h["sha256"]), (name, key, what)


def test_cases_are_the_recorded_ones(recorded):
    runs = recorded[0]
    assert runs["runs"] == mc.RUNS and sorted(k for k in runs if k != "runs") == sorted(mc.CASES)
    for name in mc.CASES:
        text = mc.case_text(name)
        assert hashlib.sha256(text.encode("latin1")).hexdigest() == runs[name]["sha256"], name
    for f in os.listdir(ACE):
        assert os.path.getsize(os.path.join(ACE, f)) < (1 << 20), f


def test_shapes_hold_what_they_promise(cases):
    m = cases["shapes"]
    lay = {r["id"]: (af, n, text) for r, (af, n, text) in zip(ref.sorted_records(m), ref.layout(m))}
    for want in (1, 49, 51, 99, 100, 101, 249, 270, 406):          # (50: twin_a and twin_b below)
        assert lay["len%d" % want][1] == want
    assert lay["no_columns"][1] == 0 and lay["twin_a"][1] == lay["twin_b"][1] == 50
    order = [r["id"] for r in ref.sorted_records(m)]
    assert order.index("twin_b") < order.index("twin_a") and order.index("first_gap_ins") < order.index("first_gap_long")
    assert lay["first_gap_none"][2].startswith("***") and lay["first_gap_ins"][2].startswith("A**") and lay["first_gap_long"][2].startswith("AC*")
    assert {r["seg"] for r in m.rec} == set("afbn") and {r["rc"] for r in m.rec} == {0, 1}
    assert min(r["start"] for r in m.rec) == 0 and max(r["end"] for r in m.rec) == m.L - 1
    assert any("-" in r["seq"] for r in m.rec) and any("-" in s for r in m.rec for _, s in r["ins"])
    assert [len(r["seq"]) - (r["end"] - r["start"] + 1) for r in m.rec if r["id"] == "long_seq"] == [5]
    assert max(len(r["ins"]) for r in m.rec) >= 30
    c = cases["column300"]
    assert len(c.rec) == 2000 and int(c.gaps.max()) == 300
    assert cases["empty"].rec == [] and mc.make_case("gaps0").gaps[0] > 0


@pytest.mark.parametrize("name", mc.CASES)
def test_restatement_reproduces_the_reference(recorded, cases, name):
    m = cases[name]
    checked = 0
    for key, args in mc.RUNS.items():
        out, written = ref.expected(m, key, args)
        if out is not None:
            check(recorded, name, key, "stdout", out)
            checked += 1
        if written is not None:
            check(recorded, name, key, "file", written)
            checked += 1
    assert checked == 5


@pytest.mark.parametrize("name", mc.CASES + mc.SCAN_EDGES)
def test_host_build_of_the_kernels_code_agrees(driver, cases, name, tmp_path):
    m = cases[name]
    path = str(tmp_path / "in.maln")
    with open(path, "w", encoding="latin1") as f:
        f.write(ms.MA_HEADER + mc.case_text(name))
    got = subprocess.run([driver, path, "ace"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert got.returncode == 0, got.stderr.decode()[-2000:]
    want = []
    for r, (af, n, text) in zip(ref.sorted_records(m), ref.layout(m)):
        want.append("%d %d\n%s" % (af, n + len(r["seq"]) - (r["end"] - r["start"] + 1), ref.lines50(text)))
    want = "".join(want).encode("latin1")
    if got.stdout != want:
        at = next((i for i, (x, y) in enumerate(zip(got.stdout, want)) if x != y), min(len(got.stdout), len(want)))
        pytest.fail(f"{name}: byte {at}: {got.stdout[max(0, at - 40):at + 20]!r} instead of {want[max(0, at - 40):at + 20]!r}")
    for code, new_id in ((1, None), (2, "my_contig")):
        got = subprocess.run([driver, path, "rewrite", str(code)] + ([new_id] if new_id else []), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert got.returncode == 0, got.stderr.decode()[-2000:]
        assert got.stdout == ref.rewrite(m, code, new_id).encode("latin1"), (name, code)


def test_refused_file_is_refused_on_the_host(driver, tmp_path):
    path = str(tmp_path / "gaps0.maln")
    with open(path, "w", encoding="latin1") as f:
        f.write(ms.MA_HEADER + mc.case_text("gaps0"))
    got = subprocess.run([driver, path, "ace"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert got.returncode == 1 and got.stdout == b""
    with pytest.raises(AssertionError):
        ref.ace(mc.make_case("gaps0"))


def test_ace_symbols_declared_and_exported():
    import mia_amd
    hdr = open(os.path.join(ROOT, "include", "mia_hip.h")).read()
    declared = set(re.findall(r"\b(mia_hip_[a-z_0-9]+)\s*\(", hdr))
    lib = mia_amd.lib()
    for sym in ("mia_hip_ma_ace", "mia_hip_get_ma_ace"):
        assert sym in declared, sym
        assert sym in mia_amd.exported_symbols(), sym
        assert hasattr(lib, sym), sym
    assert hasattr(mia_amd.MiaHip, "ma_ace")
