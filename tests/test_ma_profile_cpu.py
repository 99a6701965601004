"""The substitution profile (ma_hip -f 9, -f 91) without a GPU.  The reference's `ma` has no such report, so no recording can pin
it: the rule of tests/ma_profile_ref.py (written from DESIGN.md's text) is held to two identities with the numpy tally of
maln_synth, which tests/test_ma_synth_cpu.py holds to the reference's own `ma -f 41`; the matrix text is read back by a restatement
of the reference's read_pssm and, where the compiled reference is there, by mia itself.  The code k_ma_profile runs per lane
(csrc/ma_profile_body.h) is compiled for the host into tests/ma_profile_driver.cpp, with -fsanitize=address,undefined where g++ has
that runtime, run as a program of its own, and must make the bins of the restatement."""
import copy
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import ma_profile_ref as ref
import maln_ace_cases as mc
import maln_profile_cases as pc
import maln_sam_cases as sc
import maln_synth as ms
from conftest import GOLDEN, ROOT

MALN = os.path.join(GOLDEN, "maln")
FILES = tuple(sorted(f for f in os.listdir(MALN) if not f.endswith(".json")))
OTHERS = tuple("ace:" + n for n in mc.CASES if n not in mc.FIXTURES) + tuple("synth:" + n for n in ms.CASES) + tuple("sam:" + n for n in sc.CASES) + \
    tuple("file:" + f for f in FILES)
NAMES = tuple("prof:" + n for n in pc.CASES) + OTHERS
REF_MIA = os.path.join(ROOT, "oracle", "_ref", "mia")
_made, _prof = {}, {}


def case(name):
    if name not in _made:
        kind, key = name.split(":", 1)
        _made[name] = ms.parse_maln(mc.fixture_text(key)) if kind == "file" else \
            {"ace": mc.make_case, "synth": ms.make_case, "sam": sc.make_case, "prof": pc.make_case}[kind](key)
    return _made[name]


def prof(name, use_dropped):
    if (name, use_dropped) not in _prof:
        _prof[(name, use_dropped)] = ref.profile(case(name), use_dropped)
    return _prof[(name, use_dropped)]


def columns_only(m):
    """the records cut off behind column L - 1 and without their inserts: what the tally's words of columns 0 .. L-1 are made of"""
    t = copy.copy(m)
    t.rec = []
    for r in m.rec:
        r = dict(r)
        r["end"] = min(r["end"], m.L - 1)
        r["ins"] = []
        t.rec.append(r)
    return t


@pytest.mark.parametrize("name", OTHERS)
def test_the_restatement_against_the_tally(name):
    """Every record used.  Coverage: every column below L counts once, in count, del or bad_code.  Scores: a column that is no '-'
    adds RPSM or FPSM[d][k][j], k = A .. T, to the tally's four score words; RPSM is the mirror of FPSM, so in the read's orientation
    that is FPSM[d'][k'][j'] summed over k' -- what the profile's column sums weigh.  Both hold on every case: none of them has a depth
    code outside A .. _ or a lower-case character in SEQ (the tally reads a lower-case base as N, the profile as the base)."""
    m = case(name)
    assert not any("a" <= ch <= "z" for r in m.rec for ch in r["seq"][:r["end"] - r["start"] + 1])
    count, dele, bad, beyond = prof(name, True)
    t = ms.restate(columns_only(m))
    assert bad == 0
    assert int(count.sum() + dele.sum()) + bad == int(t.cols[5].sum()), "coverage"
    assert beyond == sum(max(0, r["end"] - max(r["start"], m.L) + 1) for r in m.rec)
    assert np.array_equal(m.rpsm, ms.revcom_pssm(m.fpsm))
    weight = m.fpsm[:, :4, :].astype(np.int64).sum(axis=1)                 # [d][j]: the four rows A .. T
    assert int((count.sum(axis=1) * weight).sum()) == int(t.cols[6:10].sum()), "scores"


def test_cases_hold_what_they_promise():
    m = case("prof:prof_classes")
    for rc in (0, 1):
        half = copy.copy(m)
        half.rec = [r for r in m.rec if r["rc"] == rc]
        count, dele, bad, beyond = ref.profile(half, True)
        assert (count > 0).all() and (dele > 0).all() and bad == 0 and beyond == 0
        count, dele, _, _ = ref.profile(half, False)
        assert (count > 0).all() and (dele > 0).all()
    text = m.ref_seq + "".join(r["seq"] for r in m.rec)
    assert any("a" <= ch <= "z" for ch in m.ref_seq) and any("a" <= ch <= "z" for r in m.rec for ch in r["seq"])
    assert "N" in text and set("RYKMSWBDHV") <= set(text) and any(r["dr"] for r in m.rec) and 200 <= len(m.rec) and all(40 <= len(r["seq"]) <= 60 for r in m.rec)
    count, dele, bad, beyond = prof("prof:prof_one_bin", False)
    assert count[15, 0, 0] == count.sum() >= 70000 and count[15, 0, 0] > 65535 and dele.sum() == 0 and not any(r["rc"] for r in case("prof:prof_one_bin").rec)
    for T in pc.EDGE_T:
        e = case("prof:prof_edges_%d" % T)
        lens = [r["end"] - r["start"] + 1 for r in e.rec]
        offs = np.concatenate([[0], np.cumsum(lens)]).tolist()
        assert offs[-1] == T and lens[0] == 1
        assert all(b in offs for b in (pc.LANE, 64, 2 * pc.WAVE, pc.WG) if b < T)
        if T > 1200:
            k = offs.index(900)
            assert lens[k] == 300 and offs[k] < pc.WAVE < offs[k + 1]
            starts = [r["start"] for r in e.rec]
            assert starts != sorted(starts)
    assert {pc.LANE - 1, pc.LANE, pc.LANE + 1, 63, 64, 65, pc.WAVE - 1, pc.WAVE, pc.WAVE + 1, pc.WG - 1, pc.WG, pc.WG + 1, 1} <= set(pc.EDGE_T)
    t = case("prof:prof_tail")
    count, dele, bad, beyond = prof("prof:prof_tail", True)
    assert beyond == 4 and bad == 9 and {"@", "`", "~"} <= set("".join(r["smp"] for r in t.rec)) and chr(ord("A") + 31) == "`"
    assert any(r["seq"] and set(r["seq"]) == {"-"} for r in t.rec) and any(r["end"] == t.L for r in t.rec)
    # a bad code sits on a '-' column in this case; the one of bad_on_base does not
    assert all(r["seq"][c] == "-" for r in t.rec for c, ch in enumerate(r["smp"]) if not "A" <= ch <= "_")
    assert any(r["seq"][c] != "-" for r in pc.bad_on_base().rec for c, ch in enumerate(r["smp"]) if not "A" <= ch <= "_")
    assert case("prof:prof_empty").rec == [] and all(r["dr"] for r in case("prof:prof_all_dropped").rec)
    count, dele, bad, beyond = prof("prof:prof_all_dropped", False)
    assert count.sum() + dele.sum() + bad + beyond == 0 and prof("prof:prof_all_dropped", True)[0].sum() > 0


@pytest.mark.parametrize("name", ["prof:prof_classes", "prof:prof_tail", "prof:prof_empty", "synth:codes_anc", "file:fix_c.1"])
@pytest.mark.parametrize("alpha", [1.0, 0.25])
def test_matrix_is_read_back(name, alpha):
    m = case(name)
    count = prof(name, False)[0]
    sm = ref.read_pssm(ref.matrix(m, alpha, prof=prof(name, False)))
    want = np.array(ref.scores(count, alpha), np.int64)
    assert np.array_equal(sm[:, :4, :4], want)
    assert (sm[:, :4, 4] == -100).all() and (sm[:, 4, :] == -10).all()         # src/io.c:443-448
    assert want.min() >= -32000 and want.max() <= 200
    # inside a row that has counts: more counts of a pair, no lower score
    for d in range(31):
        for i in range(4):
            row = count[d, i, :4]
            if row.sum() == 0:
                continue
            order = np.argsort(row, kind="stable")
            assert all(want[d, i, a] <= want[d, i, b] for a, b in zip(order, order[1:]))


def test_zero_count_row_is_flat_and_the_unit_is_the_references():
    assert [ref.score([0, 0, 0, 0], 2, j, 1.0) for j in range(4)] == [-600, -600, 200, -600]
    text = ref.matrix(case("prof:prof_empty"))
    flat = ms.flat_pssm()
    assert np.array_equal(ref.read_pssm(text), flat)
    assert ref.score([10 ** 9, 0, 0, 0], 0, 0, 1.0) == 200                     # 100 * log2(1 / 0.25)
    assert ref.score([1, 1, 1, 1], 0, 3, 1.0) == 0                              # a quarter each
    assert ref.score([0, 0, 0, 2 ** 62], 3, 0, 1.0) == -6000                    # 100 * log2(4 / (2^62 + 4))
    assert ref.score([0, 0, 0, 2 ** 62], 3, 0, ref.MIN_ALPHA) >= -32000
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-61, 1e61):
        with pytest.raises(ValueError):
            ref.matrix(case("prof:prof_empty"), bad)
    lines = ref.table(case("prof:prof_empty")).split("\n")
    assert lines[0] == "# ma_hip substitution profile: 0 records, 0 columns, 0 bad depth codes, 0 columns beyond the reference"
    assert [ln.split("\t")[0] for ln in lines[2:33]] == ref.LABELS and all(ln.split("\t")[1:] == ["0"] * 18 for ln in lines[2:33]) and lines[33:] == [""]
    shipped = [ln[len("# Matrix for position: "):] for ln in open(os.path.join(GOLDEN, "ancient.submat.txt")).read().split("\n") if ln.startswith("#")]
    assert shipped == ref.LABELS


@pytest.mark.skipif(not os.path.exists(REF_MIA), reason="the compiled reference is not here")
def test_the_reference_runs_with_the_matrix(tmp_path):
    path = str(tmp_path / "own.submat.txt")
    with open(path, "w") as f:
        f.write(ref.matrix(case("synth:codes_anc"), 1.0))
    r = subprocess.run([REF_MIA, "-r", os.path.join(GOLDEN, "tr1.fna"), "-f", os.path.join(GOLDEN, "tf.fna"), "-s", path], cwd=str(tmp_path),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr[-500:]


# ---- csrc/ma_profile_body.h on the host -------------------------------------------------------------------------------------------
def sanitizer_flags(tmp):
    """-fsanitize=address,undefined if a program built with it links and runs here"""
    src, exe = tmp / "probe.cpp", tmp / "probe"
    src.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    ok = subprocess.run(["g++"] + flags + ["-o", str(exe), str(src)], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode == 0
    return flags if ok and subprocess.run([str(exe)]).returncode == 0 else []


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ma_profile")
    flags = sanitizer_flags(tmp)
    print("ma_profile_driver: sanitizers", "on" if flags else "not available: compiled without")
    exe = tmp / "ma_profile_driver"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-g"] + flags + ["-o", str(exe), os.path.join(ROOT, "tests", "ma_profile_driver.cpp")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()
    return str(exe)


def bin_of(e):
    """count[31][5][5] | del[31] | bad_code | beyond as one list of 808"""
    if e[0] == "count":
        return (e[1] * 5 + e[2]) * 5 + e[3]
    return 775 + e[1] if e[0] == "del" else 806 if e[0] == "bad_code" else 807


def test_every_character_code_and_strand(driver, tmp_path):
    """the table of the restatement: every byte as the reference's character and every byte as SEQ's against a set of the other that
    holds every class in both cases, under depth codes at and beside every edge; that set squared under every byte as the depth code;
    each on both strands; and columns beyond the reference"""
    few = "ACGTacgtNnRyXx-.@`~ \x00\xff"
    codes = "@ABOPQ^_`~\x00\xff"
    every = [chr(b) for b in range(256)]
    rows = []
    for refs, seqs, smps in ((every, few, codes), (few, every, codes), (few, few, every)):
        for rc in (0, 1):
            for a in refs:
                for s in seqs:
                    for c in smps:
                        rows.append((rc, a, s, c, ref.event(1, a, 0, 0, s, c, bool(rc))))
    for rc in (0, 1):
        for s in few:
            for c in codes:
                rows.append((rc | 2, "A", s, c, ref.event(1, "A", 1, 0, s, c, bool(rc))))
    path = tmp_path / "table.bin"
    path.write_bytes(b"".join(struct.pack("<BBBBh", fl, ord(a), ord(s), ord(c), bin_of(e)) for fl, a, s, c, e in rows))
    got = subprocess.run([driver, "bins", str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert got.returncode == 0, got.stderr.decode("latin1")[-2000:]
    assert int(got.stdout) == len(rows) > 300000


@pytest.mark.parametrize("name", tuple("prof:" + n for n in pc.CASES) + ("sam:sam_shapes", "ace:shapes", "synth:edge257", "synth:codes_anc", "file:fix_c.1"))
def test_host_build_of_the_kernels_walk_agrees(driver, name, tmp_path):
    m = case(name)
    path = str(tmp_path / "in.maln")
    with open(path, "w", encoding="latin1") as f:
        f.write(ms.MA_HEADER + ms.write_maln(m))
    for use_dropped in (False, True):
        got = subprocess.run([driver, "profile", path] + (["A"] if use_dropped else []), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert got.returncode == 0, got.stderr.decode("latin1")[-2000:]
        count, dele, bad, beyond = prof(name, use_dropped)
        want = [len(ref.counted(m, use_dropped))] + count.reshape(-1).tolist() + dele.tolist() + [bad, beyond]
        assert [int(x) for x in got.stdout.split()] == want, (name, use_dropped)


def test_host_scores_and_labels(driver, tmp_path):
    rows = [(1.0, 0, 0, 0, 0, 0), (1.0, 2, 0, 0, 0, 0), (1.0, 0, 100, 3, 1, 40), (0.25, 1, 0, 7, 0, 0), (0.25, 3, 1, 1, 1, 1), (1.0, 3, 0, 0, 0, 2 ** 62),
              (1e-60, 0, 0, 0, 0, 2 ** 62), (3.5, 2, 123456789, 5, 17, 99999), (0.0, 0, 1, 1, 1, 1), (1e-61, 0, 1, 1, 1, 1), (1e61, 0, 1, 1, 1, 1)]
    count = prof("prof:prof_classes", False)[0]
    rows += [(a, i) + tuple(int(x) for x in count[d, i, :4]) for a in (1.0, 0.25) for d in range(31) for i in range(4)]
    path = tmp_path / "rows.txt"
    path.write_text("".join("%r %d %d %d %d %d\n" % r for r in rows))
    got = subprocess.run([driver, "scores", str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert got.returncode == 0, got.stderr.decode("latin1")[-2000:]
    want = []
    for a, i, *c in rows:
        ok = np.isfinite(a) and ref.MIN_ALPHA <= a <= ref.MAX_ALPHA
        want.append("%d %d %d %d" % tuple(ref.score(c, i, j, a) for j in range(4)) if ok else "refused")
    assert got.stdout.decode().split("\n") == want + ref.LABELS + [""]


def test_profile_symbols_declared_and_exported():
    import mia_amd
    hdr = open(os.path.join(ROOT, "include", "mia_hip.h")).read()
    declared = set(re.findall(r"\b(mia_hip_[a-z_0-9]+)\s*\(", hdr))
    lib = mia_amd.lib()
    for sym in ("mia_hip_ma_profile", "mia_hip_get_ma_profile"):
        assert sym in declared, sym
        assert sym in mia_amd.exported_symbols(), sym
        assert hasattr(lib, sym), sym
    assert hasattr(mia_amd.MiaHip, "ma_profile")
    assert {"k_ma_profile"} <= set(mia_amd.MiaHip.STAGES)
    assert os.path.exists(os.path.join(ROOT, "mapping-iterative-assembler_amd", "csrc", "ma_profile_body.h"))
