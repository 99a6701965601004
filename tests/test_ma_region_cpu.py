"""The region view of ma (-f 6) without a GPU: the code the region kernels run per record (csrc/ma_region_body.h, MIA_HD:
the overlap test and the rendering of a row) is compiled for the host into tests/ma_region_driver.cpp, which reads a
.maln through ma_hip's own reader (host/maln_text.h: record order, -R parsing, clamping, row labels) and prints the
record lines.  They must be the record lines of the reference's `ma -f 6` for every recorded region of every committed
.maln (tests/golden/ma_region, written by tools/make_ma_region_goldens.py from oracle/_ref/ma)."""
import gzip
import json
import os
import re
import subprocess

import pytest

from conftest import GOLDEN, ROOT

HEADER = "/* map_alignment [V1.0] */ golden\n"
REGION = os.path.join(GOLDEN, "ma_region")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("ma_region") / "ma_region_driver"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-o", str(exe), os.path.join(ROOT, "tests", "ma_region_driver.cpp")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()
    return str(exe)


def recorded_runs():
    """{maln name: {run key: arguments}} of tests/golden/ma_region/runs.json: the runs every file gets, and "f6.<tag>" and
    "f61.<tag>" for each of its regions"""
    with open(os.path.join(REGION, "runs.json")) as f:
        rec = json.load(f)
    runs = {}
    for name, regions in rec["regions"].items():
        runs[name] = dict(rec["common"])
        for tag, arg in regions.items():
            for fmt in ("6", "61"):
                runs[name][f"f{fmt}.{tag}"] = ["-f", fmt] + (["-R", arg] if arg is not None else [])
    return runs


def test_region_rows_match_the_reference_on_the_host(driver, tmp_path):
    runs = recorded_runs()
    malns = sorted(os.path.basename(p) for p in os.listdir(os.path.join(GOLDEN, "maln")) if re.search(r"\.[0-9]$", p))
    assert sorted(runs) == malns                     # every committed .maln has its recorded runs
    with gzip.open(os.path.join(REGION, "outputs.json.gz")) as f:
        outputs = json.load(f)
    checked = with_inserts = 0
    for name in malns:
        full = str(tmp_path / name)
        with open(full, "w") as f:
            f.write(HEADER + open(os.path.join(GOLDEN, "maln", name)).read())
        small = outputs[name]
        for key, args in sorted(runs[name].items()):
            if not key.startswith("f6.R"):
                continue
            assert key in small, (name, key)          # region views are short: never pinned by hash only
            region = [args[args.index("-R") + 1]] if "-R" in args else []
            out = subprocess.run([driver, full] + region, check=True, stdout=subprocess.PIPE, timeout=120).stdout
            lines = small[key].encode("latin1").split(b"\n")
            assert lines[-1] == b"" and lines[1].startswith(b"Consensus"), (name, key)
            assert out == b"".join(l + b"\n" for l in lines[2:-1]), (name, key)
            checked += 1
            with_inserts += 1 if b"-" in lines[0][21:] else 0
    assert checked == sum(1 for r in runs.values() for k in r if k.startswith("f6.R")) and checked >= 7 * len(malns)
    assert with_inserts >= 3                         # regions whose reference line has insert columns


def test_region_symbols_declared_and_exported():
    import mia_amd
    hdr = open(os.path.join(ROOT, "include", "mia_hip.h")).read()
    declared = set(re.findall(r"\b(mia_hip_[a-z_0-9]+)\s*\(", hdr))
    lib = mia_amd.lib()
    for sym in ("mia_hip_ma_region", "mia_hip_get_ma_region"):
        assert sym in declared, sym
        assert sym in mia_amd.exported_symbols(), sym
        assert hasattr(lib, sym), sym
    assert os.path.exists(os.path.join(ROOT, "mapping-iterative-assembler_amd", "csrc", "ma_region_body.h"))
