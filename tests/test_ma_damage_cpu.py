"""The deaminated-fragment filter (ma_hip -D, -e, -S, -f 95) without a GPU.  tests/ma_damage_ref.py restates the rule of DESIGN.md
("Deaminated fragments") as a loop over records and columns and a dictionary of molecules; here it is held to a table written out by
hand, to the substitution profile's own restatement (the hits are bins of that profile), and to itself under a permutation of the
records.  The code the kernels run per lane (csrc/ma_damage_body.h) is compiled for the host into tests/ma_damage_driver.cpp, with
-fsanitize=address,undefined where g++ has that runtime, run as a program of its own: its stretches must agree with its own walk
record by record and with the restatement for every case, use mask, library, N and ends mode."""
import collections
import os
import re
import subprocess

import numpy as np
import pytest

import ma_damage_ref as ref
import ma_dedup_ref
import ma_profile_ref
import maln_damage_cases as dc
import maln_synth as ms
from conftest import ROOT

HAND_IDS = ["h0", "h1", "h2", "h3", "h4", "h5", "h6", "w_f", "w_b", "x_b", "x_f", "o_f", "d0"]
#             h0 h1 h2  h3 h4 h5 h6 w_f w_b x_b x_f o_f d0
HAND_POS = {False: ([1, 3, 15, 0, 0, 1, 0, 3, 0, 0, 0, 1, 1], [0, 0, 1, 0, 0, 3, 0, 0, 0, 1, 0, 0, 0]),
            True: ([1, 3, 15, 0, 0, 1, 0, 3, 0, 0, 0, 1, 1], [0, 0, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0])}
# keep per (library, N, mode), a character per record in the order of HAND_IDS
HAND_KEEP = {
    (False, 1, "any"): "1010010001111", (False, 1, "5"): "1000010000011", (False, 1, "3"): "0010000001100", (False, 1, "both"): "0000000000000",
    (False, 3, "any"): "1110010111111", (False, 3, "5"): "1100010110011", (False, 3, "3"): "0010010001100", (False, 3, "both"): "0000010000000",
    (False, 15, "any"): "1110010111111", (False, 15, "5"): "1110010110011", (False, 15, "3"): "0010010001100", (False, 15, "both"): "0010010000000",
    (True, 1, "any"): "1000010000011", (True, 1, "5"): "1000010000011", (True, 1, "3"): "0000000000000", (True, 1, "both"): "0000000000000",
    (True, 3, "any"): "1101010110011", (True, 3, "5"): "1100010110011", (True, 3, "3"): "0001000000000", (True, 3, "both"): "0000000000000",
    (True, 15, "any"): "1111010110011", (True, 15, "5"): "1110010110011", (True, 15, "3"): "0001000000000", (True, 15, "both"): "0000000000000",
}


def test_the_hand_table():
    m, _ = dc.case("hand")
    assert [r["id"] for r in m.rec] == HAND_IDS
    mate = ma_dedup_ref.pair_halves(m.rec)
    assert mate.tolist() == [-1, -1, -1, -1, -1, -1, -1, 8, 7, 10, 9, -2, -1]
    for ss in (False, True):
        for (lib, n_pos, mode), keep in HAND_KEEP.items():
            if lib != ss:
                continue
            pos5, pos3, got, hist, n_mol, n_kept, orphans = ref.damage(m, n_pos, mode, ss)
            assert (pos5.tolist(), pos3.tolist()) == HAND_POS[ss], ss
            assert "".join(str(k) for k in got) == keep, (ss, n_pos, mode)
            assert (n_mol, n_kept, orphans) == (11, keep.count("1"), 1)
    hist = ref.damage(m, 3, "any", False)[3]
    want = np.zeros((2, 16, 16), np.int64)
    for strand, m5, m3, k in ((0, 1, 0, 3), (0, 3, 0, 2), (0, 15, 1, 1), (0, 0, 0, 3), (1, 1, 3, 1), (0, 0, 1, 1)):
        want[strand, m5, m3] = k                             # h0 o_f d0 | h1 w | h2 | h3 h4 h6 | h5 | x
    assert np.array_equal(hist, want)
    # the dropped record left out: one molecule less in class (1, 0)
    use = np.array([0 if r["dr"] else 1 for r in m.rec], np.uint8)
    got = ref.damage(m, 3, "any", False, use)
    want[0, 1, 0] = 2
    assert np.array_equal(got[3], want) and got[4] == 10 and got[0][12] == 0 and got[2][12] == 0


def test_table_text_from_a_hist_written_by_hand():
    hist = np.zeros((2, 16, 16), np.int64)
    hist[0, 1, 0], hist[0, 3, 2], hist[1, 0, 15], hist[1, 0, 0], hist[0, 15, 15] = 4, 2, 1, 7, 1
    text = ref.table_of(hist, 3, 20, False).split("\n")
    assert text[0] == "# ma_hip damage classes: 15 molecules, 3 orphan halves, 20 records, library ds"
    assert text[1] == "# N\t5p+\t3p+\tboth+\teither+\t5p-\t3p-\tboth-\teither-\t5p\t3p\tboth\teither"
    assert text[2] == "1\t4\t0\t0\t4\t0\t0\t0\t0\t4\t0\t0\t4"
    assert text[3] == "2\t4\t2\t0\t6\t0\t0\t0\t0\t4\t2\t0\t6"
    assert text[4] == "3\t6\t2\t2\t6\t0\t0\t0\t0\t6\t2\t2\t6"
    assert text[16] == "15\t7\t3\t3\t7\t0\t1\t0\t1\t7\t4\t3\t8"
    assert len(text) == 18 and text[17] == ""
    assert ref.table_of(np.zeros((2, 16, 16), np.int64), 0, 0, True).split("\n")[0].endswith("0 records, library ss")
    empty = ref.table(dc.case("empty")[0])
    assert empty.split("\n")[2:17] == ["%d" % n + "\t0" * 12 for n in range(1, 16)]


@pytest.mark.parametrize("name", dc.CASES)
def test_hits_are_bins_of_the_substitution_profile(name):
    """the multiset of the restatement's hits equals the bins count[k-1][C][T], count[31-k][G][A] (ds) / count[31-k][C][T] (ss) of
    tests/ma_profile_ref.py on the same records and the same selection"""
    m, _ = dc.case(name)
    for use in dc.uses(name):
        sub = ms.Maln()
        sub.L, sub.ref_seq = m.L, m.ref_seq
        sub.rec = [dict(r, dr=0) for k, r in enumerate(m.rec) if use is None or use[k]]
        count = ma_profile_ref.profile(sub)[0]
        for ss in (False, True):
            found = collections.Counter((end, k) for _r, end, k in ref.hits(m, use, ss))
            for k in range(1, 16):
                assert found[("5", k)] == count[k - 1, 1, 3], (name, ss, k)
                assert found[("3", k)] == (count[31 - k, 1, 3] if ss else count[31 - k, 2, 0]), (name, ss, k)


def test_cases_hold_what_they_promise():
    m, _ = dc.case("mirror")
    pos5, pos3 = ref.positions(m)
    assert len(dc.MIRROR_PAIRS) == 12 and any(pos5[a] for a, _ in dc.MIRROR_PAIRS) and any(pos3[a] for a, _ in dc.MIRROR_PAIRS)
    for a, b in dc.MIRROR_PAIRS:
        assert (pos5[a], pos3[a]) == (pos5[b], pos3[b]), (a, b)
    for name, want in (("edge_before", 4), ("edge_behind", 11)):
        m, _ = dc.case(name)
        at = [r["id"] for r in m.rec].index("straddle")
        off = sum(len(r["seq"]) for r in m.rec[:at])
        assert off < dc.CHUNK < off + 31 and ref.hits(m) == [(at, "5", want)]
        assert (off + want - 1 < dc.CHUNK) == (name == "edge_before")
    m, _ = dc.case("odd")
    pos5, pos3 = ref.positions(m)
    by_id = {r["id"]: k for k, r in enumerate(m.rec)}
    assert [int(pos5[by_id[i]]) for i in ("dash", "lower_seq", "lower_ref", "ref_n", "bad_code", "short")] == [0, 2, 3, 0, 5, 11]
    assert [int(pos3[by_id[i]]) for i in ("beyond", "last_col", "short")] == [0, 1, 0]
    m, masks = dc.case("wrap")
    by_id = {r["id"]: k for k, r in enumerate(m.rec)}
    got = ref.damage(m, 1, "any")
    for tag, m5, m3 in (("front", 1, 0), ("back", 0, 1), ("both", 3, 3), ("none", 0, 0)):
        f, b = by_id[tag + "0_f"], by_id[tag + "0_b"]
        assert (max(got[0][f], got[0][b]), max(got[1][f], got[1][b])) == (m5, m3), tag
        assert got[2][f] == got[2][b] == (1 if 0 < m5 <= 1 or 0 < m3 <= 1 else 0), tag
    assert got[2][by_id["back_first_f"]] == got[2][by_id["back_first_b"]] == 1
    assert got[6] == 6                                       # orphan_f, strands_f, strands_b, twice_f twice, twice_b
    silenced = ref.damage(m, 1, "any", use=masks[0])
    assert silenced[2][by_id["front0_f"]] == silenced[2][by_id["front0_b"]] == 0 and silenced[4] == got[4]
    gone = ref.damage(m, 1, "any", use=masks[1])
    assert gone[4] == got[4] - 2 and gone[6] == got[6] - 1
    assert ref.damage(m, 1, "any", use=masks[2])[4:] == (0, 0, 0)
    m, _ = dc.case("pile_3000")
    hist = ref.damage(m, 1, "both")[3]
    assert hist[0, 1, 1] == 3000 and hist.sum() == 3000


@pytest.mark.parametrize("name", ("hand", "wrap", "mixed", "offsets"))
def test_a_permutation_of_the_records_permutes_the_result(name):
    m, _ = dc.case(name)
    perm = ms.Rng(78).permutation(len(m.rec)).tolist()
    moved = ms.Maln()
    moved.L, moved.ref_seq, moved.gaps = m.L, m.ref_seq, m.gaps
    moved.rec = [m.rec[p] for p in perm]
    for n_pos, mode, ss in ((1, "any", False), (3, "both", False), (2, "3", True)):
        a, b = ref.damage(m, n_pos, mode, ss), ref.damage(moved, n_pos, mode, ss)
        for k in range(3):
            assert np.array_equal(b[k], a[k][perm]), (name, k)
        assert a[4:] == b[4:]
        assert np.array_equal(a[3], b[3])
    if name == "mixed":
        rev, _ = dc.case("mixed_reversed")
        assert [r["id"] for r in rev.rec] == [r["id"] for r in m.rec][::-1]
        a, b = ref.damage(m, 3, "any"), ref.damage(rev, 3, "any")
        assert np.array_equal(a[3], b[3]) and np.array_equal(a[2], b[2][::-1]) and a[4:] == b[4:]


def sanitizer_flags(tmp):
    """-fsanitize=address,undefined if g++ can link and run such a program here, else nothing"""
    src, exe = tmp / "probe.cpp", tmp / "probe"
    src.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    ok = subprocess.run(["g++"] + flags + ["-o", str(exe), str(src)], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode == 0
    return flags if ok and subprocess.run([str(exe)]).returncode == 0 else []


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ma_damage")
    flags = sanitizer_flags(tmp)
    print("ma_damage_driver: sanitizers", "on" if flags else "not available: compiled without")
    exe = tmp / "ma_damage_driver"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-g"] + flags + ["-o", str(exe), os.path.join(ROOT, "tests", "ma_damage_driver.cpp")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()
    return str(exe)


@pytest.mark.parametrize("name", dc.CASES)
def test_host_build_of_the_kernels_body_agrees(driver, name, tmp_path):
    m, _ = dc.case(name)
    f = ms.flatten(m)
    mate = ma_dedup_ref.pair_halves(m.rec)
    for which, use in enumerate(dc.uses(name)):
        path = str(tmp_path / ("in%d.txt" % which))
        with open(path, "w", encoding="latin1") as out:
            out.write("%d %d %d\n%s\n>%s\n>%s\n" % (m.L, len(m.rec), f["col_off"][-1], m.ref_seq, f["seq"].tobytes().decode("latin1"), f["smp"].tobytes().decode("latin1")))
            for r in range(len(m.rec)):
                out.write("%d %d %d %d %d\n" % (f["start"][r], f["revcom"][r], 1 if use is None else use[r], mate[r], f["col_off"][r + 1]))
        got = subprocess.run([driver, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert got.returncode == 0, got.stderr.decode("latin1")[-2000:]
        lines = got.stdout.decode().split("\n")
        assert len(lines) == 2 * (2 + 3 * 16) + 1
        at = 0
        for ss in (False, True):
            pos = ref.positions(m, use, ss)
            assert np.array_equal(np.array(lines[at].split()[1:], np.uint8), pos[0]), (name, which, ss)
            assert np.array_equal(np.array(lines[at + 1].split()[1:], np.uint8), pos[1]), (name, which, ss)
            at += 2
            for n_pos in ref.GRID_N:
                for k, mode in enumerate(ref.MODES):
                    _p5, _p3, keep, hist, n_mol, n_kept, orphans = ref.damage(m, n_pos, mode, ss, use, mate, pos)
                    assert [int(x) for x in lines[at].split()] == [n_pos, k, n_mol, n_kept, orphans], (name, which, ss, n_pos, mode)
                    assert lines[at + 1] == ("".join(str(x) for x in keep) or "-"), (name, which, ss, n_pos, mode)
                    pairs = [int(x) for x in lines[at + 2].split()[1:]]
                    sparse = np.zeros(512, np.int64)
                    sparse[pairs[0::2]] = pairs[1::2]
                    assert np.array_equal(sparse.reshape(2, 16, 16), hist), (name, which, ss, n_pos, mode)
                    at += 3


def test_damage_symbols_declared_exported_and_bound():
    import mia_amd
    hdr = open(os.path.join(ROOT, "include", "mia_hip.h")).read()
    declared = set(re.findall(r"\b(mia_hip_[a-z_0-9]+)\s*\(", hdr))
    lib = mia_amd.lib()
    for sym in ("mia_hip_ma_damage", "mia_hip_get_ma_damage"):
        assert sym in declared, sym
        assert sym in mia_amd.exported_symbols(), sym
        assert hasattr(lib, sym), sym
    assert hasattr(mia_amd.MiaHip, "ma_damage")
    stages = mia_amd.MiaHip.STAGES
    at = stages.index("k_ma_damage_hits")
    assert stages[at - 1:at + 3] == ["k_ma_sam_render", "k_ma_damage_hits", "k_ma_damage_molecules", "k_ma_profile"]
    src = open(os.path.join(ROOT, "mapping-iterative-assembler_amd", "csrc", "mia_hip.hip")).read()
    table = re.search(r"STAGE_NAMES\[STG_COUNT\] = \{(.*?)\};", src, re.S).group(1)
    assert re.findall(r'"([a-z_0-9]+)"', table) == stages
    assert len(stages) <= 32                                 # a bit per stage in mia_hip_set_stage_mask
    for f in ("ma_damage_body.h", "mia_ma_damage_kernels.h"):
        assert os.path.exists(os.path.join(ROOT, "mapping-iterative-assembler_amd", "csrc", f))
