"""DevPool and PoolLease (csrc/dev_pool.h), the temporaries of the one-off calls, without a GPU: tests/dev_pool_driver.cpp supplies counting
stand-ins for hipMalloc / hipFree (malloc / free underneath) and is built as a stand-alone program under the address and
undefined-behaviour sanitizers, so a block freed twice, used after its release or never freed ends the run.  One case per property;
every case also ends on "every block idle again, frees equal successful mallocs, each block exactly once"."""
import os
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("dev_pool") / "dev_pool_driver"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-o", str(exe), os.path.join(ROOT, "tests", "dev_pool_driver.cpp")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()
    return str(exe)


# best fit: the smallest idle block that holds the request | nothing fits: the largest idle block is freed first, then exactly the
# request is allocated | a lease out of scope (an early return out of a nest of leases too) leaves its block idle, the next equal
# request gets it back without a malloc | two live leases never share a block | a refused allocation leaves the lease empty and the
# pool usable | a moved-from lease gives nothing back, the target once | a lease taken before the pool grows returns its own block
@pytest.mark.parametrize("case", ["best_fit", "grow", "scope", "distinct", "refused", "move", "by_pointer"])
def test_dev_pool(driver, case):
    r = subprocess.run([driver, case], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    assert r.returncode == 0, r.stdout.decode()
    assert r.stdout.decode().strip().endswith("0 failed checks")


def test_header_brings_no_runtime_of_its_own():
    """the including file supplies hipMalloc / hipFree: the header itself includes nothing of HIP"""
    text = open(os.path.join(ROOT, "mapping-iterative-assembler_amd", "csrc", "dev_pool.h")).read()
    assert "#include <hip" not in text and "#include \"hip" not in text
