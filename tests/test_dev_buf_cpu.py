"""DevBuf (csrc/dev_buf.h), the owner of every device block of the context, without a GPU: tests/dev_buf_driver.cpp supplies counting
stand-ins for hipMalloc / hipFree (malloc / free underneath) and is built as a stand-alone program under the address and
undefined-behaviour sanitizers, so a block freed twice, used after its release or never freed ends the run.  One case per property;
every case also ends on "frees equal successful mallocs, each block exactly once"."""
import os
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("dev_buf") / "dev_buf_driver"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-o", str(exe), os.path.join(ROOT, "tests", "dev_buf_driver.cpp")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()
    return str(exe)


# ensure: nothing while need <= cap, exactly alloc_elems otherwise | the old block is freed before the new one is requested |
# a refused allocation leaves p == nullptr and cap == 0, and the next smaller request allocates again | move empties the source,
# destructor and release free once | alloc(0) is a valid one-element block
@pytest.mark.parametrize("case", ["ensure", "order", "failure", "move", "zero"])
def test_dev_buf(driver, case):
    r = subprocess.run([driver, case], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    assert r.returncode == 0, r.stdout.decode()
    assert r.stdout.decode().strip().endswith("0 failed checks")


def test_header_brings_no_runtime_of_its_own():
    """the including file supplies hipMalloc / hipFree: the header itself includes nothing of HIP"""
    text = open(os.path.join(ROOT, "mapping-iterative-assembler_amd", "csrc", "dev_buf.h")).read()
    assert "#include <hip" not in text and "#include \"hip" not in text
