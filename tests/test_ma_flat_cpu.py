"""The walk over the flat columns that the profile, the deaminated-fragment filter, the damage score and the end mask share
(csrc/ma_flat_body.h), without a GPU.  tests/ma_flat_driver.cpp is compiled for the host, with -fsanitize=address,undefined where g++
has that runtime, and run as a program of its own: over every stretch of its hand-made geometries, in both EVERY_POSITION forms, the
sequence of column calls (every field) and of leave calls (once per stretch and record that has a column there, `whole` as defined)
must equal a plain loop's record by record and column by column, and the EVERY_POSITION form must make exactly 16 column calls per
stretch, those at or behind T marked not live."""
import os
import subprocess

import pytest

from conftest import ROOT
from test_ma_damage_cpu import sanitizer_flags

# name: (stretches walked, one of them behind T; columns; leave calls; of them whole; columns with p >= L)
GEOMETRIES = {
    "empty": (1, 0, 0, 0, 0),
    "one_column": (2, 1, 1, 1, 0),
    "T15": (2, 15, 1, 1, 0),
    "T16": (2, 16, 1, 1, 0),
    "T17": (3, 17, 2, 0, 0),
    "seam_on_16": (3, 21, 2, 2, 0),
    "seam_on_16_inside": (4, 36, 4, 2, 0),
    "sixteen_ones": (2, 16, 16, 16, 0),
    "empty_records": (2, 7, 2, 2, 0),
    "empty_records_on_16": (3, 21, 2, 2, 0),
    "three_stretches": (4, 39, 5, 2, 0),
    "exactly_one_stretch": (4, 48, 3, 3, 0),
    "beyond_L": (2, 10, 2, 2, 1),
}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ma_flat")
    flags = sanitizer_flags(tmp)
    print("ma_flat_driver: sanitizers", "on" if flags else "not available: compiled without")
    exe = tmp / "ma_flat_driver"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-g"] + flags + ["-o", str(exe), os.path.join(ROOT, "tests", "ma_flat_driver.cpp")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()
    return str(exe)


def test_the_walk_agrees_with_a_plain_loop_on_every_stretch(driver):
    got = subprocess.run([driver], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert got.returncode == 0, got.stderr.decode("latin1")[-2000:]
    lines = got.stdout.decode().split("\n")
    assert lines[-2:] == ["ok", ""]
    seen = {}
    for line in lines[:-2]:
        name, use, *figures = line.split()
        seen[(name, int(use))] = tuple(int(x) for x in figures)
    # every geometry, with a null `use` (0) and with a `use` array that has zeros (1): the figures do not depend on the selection
    assert seen == {(name, use): figures for name, figures in GEOMETRIES.items() for use in (0, 1)}
