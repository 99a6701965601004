"""The cull's arithmetic without a GPU: csrc/cull_body.h (records per read, the links a read will emit, a block's first AlnSeq slot
from k_slot_count's raw counts) compiled with g++ into tests/cull_body_driver.cpp -- with -fsanitize=address,undefined where g++ has
that runtime, run as a program of its own -- and held against a numpy restatement.

The kernels use the same functions: k_slot_count counts with cull_records / cull_links, k_cull_records adds cull_share over its 256
threads.  The driver fills partial[] the way k_slot_count does, in exactly cull_partial_words(n) words."""
import itertools
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NS = [1, 255, 256, 257, 4095, 4096, 4097, 3 * 4096 + 17]
L = 700


def sanitizer_flags(tmp):
    """-fsanitize=address,undefined if g++ can link and run such a program here, else nothing"""
    src, exe = tmp / "probe.cpp", tmp / "probe"
    src.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    ok = subprocess.run(["g++"] + flags + ["-o", str(exe), str(src)], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode == 0
    return flags if ok and subprocess.run([str(exe)]).returncode == 0 else []


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("cull_body")
    flags = sanitizer_flags(tmp)
    print("cull_body_driver: sanitizers", "on" if flags else "not available: compiled without")
    exe = tmp / "cull_body_driver"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-g"] + flags + ["-o", str(exe), os.path.join(ROOT, "tests", "cull_body_driver.cpp")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()
    return str(exe)


def ask(driver, ref_len, sk, as_, ae, back, front):
    n = len(sk)
    text = "%d %d\n" % (ref_len, n) + "".join("%d %d %d %d %d\n" % row for row in zip(sk.tolist(), as_.tolist(), ae.tolist(), back.tolist(), front.tolist()))
    got = subprocess.run([driver], input=text.encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert got.returncode == 0, got.stderr.decode()
    rows = [tuple(int(x) for x in line.split()) for line in got.stdout.decode().split("\n") if line]
    nb = (n + 255) // 256
    assert len(rows) == n + nb
    return np.array(rows[:n], np.int64).reshape(n, 2), np.array(rows[n:], np.int64).reshape(nb, 3)


def restate(ref_len, sk, as_, ae, back, front):
    """records and links per read, as src/mia_main.c:259-276 and the cull's link rules say them"""
    end = np.where(ae > ref_len, ae - ref_len, ae)
    split = as_ > end
    rec = np.where(sk != 0, 1 + split.astype(np.int64), 0)
    links = np.where(sk != 0, (~split & (back >= 0)).astype(np.int64), (front >= 0).astype(np.int64) + (back >= 0).astype(np.int64))
    return rec, links, split


def test_the_link_predicate_on_every_combination(driver):
    # sk, split, back_slot and front_slot0 at -1 / 0 / a slot further on: the table written out, not derived
    combos = list(itertools.product([0, 1], [0, 1], [-1, 0, 9], [-1, 0, 4]))
    sk = np.array([c[0] for c in combos], np.int64)
    split = np.array([c[1] for c in combos], bool)
    as_ = np.where(split, 650, 100).astype(np.int64)
    ae = as_ + 99                                             # 650 .. 749 runs over the origin of 700 columns
    back = np.array([c[2] for c in combos], np.int64)
    front = np.array([c[3] for c in combos], np.int64)
    per_read, _ = ask(driver, L, sk, as_, ae, back, front)
    want = []
    for s, sp, b, f in combos:
        if not s:
            want.append((0, int(f >= 0) + int(b >= 0)))       # strand unknown: no record, both pass-1 pointers followed (split or not)
        elif sp:
            want.append((2, 0))                               # split now: its back pointer is overwritten, not followed
        else:
            want.append((1, int(b >= 0)))                     # the stale back pointer of a read that was split once
    assert per_read.tolist() == [list(w) for w in want]
    rec, links, sp2 = restate(L, sk, as_, ae, back, front)
    assert np.array_equal(sp2, split) and np.array_equal(per_read[:, 0], rec) and np.array_equal(per_read[:, 1], links)


def reads_of(n, seed):
    """n reads of 100 bases on 700 circular columns: about one in seven over the origin, a tenth strand-unknown, a few pointers --
    and a split read on the last lane of a wavefront, the last read of a block and of the last block of a group of sixteen"""
    rng = np.random.default_rng(seed)
    as_ = rng.integers(0, L, n).astype(np.int64)
    sk = (rng.random(n) >= 0.1).astype(np.int64)
    back = np.where(rng.random(n) < 0.05, rng.integers(0, 2 * n + 1, n), -1).astype(np.int64)
    front = np.where(rng.random(n) < 0.05, rng.integers(0, 2 * n + 1, n), -1).astype(np.int64)
    for at in (63, 255, 4095, 2 * 4096 - 1, 3 * 4096 - 1, n - 1):
        if 0 <= at < n:
            as_[at], sk[at] = 650, 1
    return sk, as_, as_ + 99, back, front


@pytest.mark.parametrize("n", NS)
def test_records_links_and_the_first_slot_of_every_block(driver, n):
    sk, as_, ae, back, front = reads_of(n, n)
    per_read, per_block = ask(driver, L, sk, as_, ae, back, front)
    rec, links, split = restate(L, sk, as_, ae, back, front)
    for at in (63, 255, 4095, n - 1):
        if 0 <= at < n:
            assert split[at] and rec[at] == 2
    assert np.array_equal(per_read[:, 0], rec) and np.array_equal(per_read[:, 1], links)
    before = np.concatenate([[0], np.cumsum(rec)])
    nb = (n + 255) // 256
    assert np.array_equal(per_block[:, 0], before[np.arange(nb) * 256])        # a block's first slot: the records of the reads before it
    assert (per_block[:, 1] == rec.sum()).all() and (per_block[:, 2] == links.sum()).all()


@pytest.mark.parametrize("n", NS)
def test_no_link_counts_as_none(driver, n):
    # the lean form of k_cull_records runs exactly where this sum is 0
    sk, as_, ae, _, _ = reads_of(n, n + 1)
    none = np.full(n, -1, np.int64)
    per_read, per_block = ask(driver, L, sk, as_, ae, none, none)
    assert not per_read[:, 1].any() and not per_block[:, 2].any()
