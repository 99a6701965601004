"""The SAM export (ma_hip -f 8) without a GPU.  The reference's `ma` has no SAM output, so no recording can pin this report: it is
held to the rule of tests/ma_sam_ref.py (written from DESIGN.md's text) and to the way back -- every record rebuilt from its SAM line.
The code the SAM kernels run per walk position and per stretch (csrc/ma_sam_body.h) is compiled for the host into
tests/ma_sam_driver.cpp, with -fsanitize=address,undefined where g++ has that runtime, run as a program of its own, and must print
the bodies and NM values of the restatement."""
import os
import re
import subprocess

import pytest

import ma_sam_ref as ref
import maln_ace_cases as mc
import maln_sam_cases as sc
import maln_synth as ms
from conftest import GOLDEN, ROOT

MALN = os.path.join(GOLDEN, "maln")
FILES = tuple(sorted(f for f in os.listdir(MALN) if not f.endswith(".json")))
# (a case of maln_ace_cases that is a committed file is taken as that file)
NAMES = tuple("ace:" + n for n in mc.CASES if n not in mc.FIXTURES) + tuple("synth:" + n for n in ms.CASES) + tuple("sam:" + n for n in sc.CASES) + \
    tuple("file:" + f for f in FILES)
# one workgroup's worth of records of each layout kernel, and the sizes beside it: held to the restatement like the rest
NAMES += tuple("ace:" + n for n in mc.SCAN_EDGES) + tuple("sam:" + n for n in sc.SCAN_EDGES)
_made = {}


def case(name):
    """(Maln, the .maln text from its MALN_NAS line on)"""
    if name not in _made:
        kind, key = name.split(":", 1)
        if kind == "file":
            text = mc.fixture_text(key)
            _made[name] = (ms.parse_maln(text), text)
        else:
            m = {"ace": mc.make_case, "synth": ms.make_case, "sam": sc.make_case}[kind](key)
            _made[name] = (m, ms.write_maln(m))
    return _made[name]


def sanitizer_flags(tmp):
    """-fsanitize=address,undefined if a program built with it links and runs here"""
    src, exe = tmp / "probe.cpp", tmp / "probe"
    src.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    ok = subprocess.run(["g++"] + flags + ["-o", str(exe), str(src)], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode == 0
    return flags if ok and subprocess.run([str(exe)]).returncode == 0 else []


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ma_sam")
    flags = sanitizer_flags(tmp)
    print("ma_sam_driver: sanitizers", "on" if flags else "not available: compiled without")
    exe = tmp / "ma_sam_driver"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-g"] + flags + ["-o", str(exe), os.path.join(ROOT, "tests", "ma_sam_driver.cpp")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()
    return str(exe)


def direct_nm(r, L, ref_seq):
    """NM counted straight from the record: '-' columns, insert characters and differing columns, all below column L"""
    s, n = r["start"], r["end"] - r["start"] + 1
    ins = ref.ins_table(r)
    nm = 0
    for c in range(min(n, L - s)):
        nm += len(ins.get(c, "").replace("-", ""))
        a, b = r["seq"][c], ref_seq[s + c]
        nm += 1 if a == "-" or ref._up(a) != ref._up(b) else 0
    return nm


@pytest.mark.parametrize("name", NAMES)
def test_lines_hold_and_rebuild_their_records(name):
    m, _ = case(name)
    text = ref.sam(m)
    lines = text.split("\n")
    assert lines[-1] == "" and lines[:3] == ["@HD\tVN:1.6\tSO:coordinate", "@SQ\tSN:%s\tLN:%d" % (m.ref_id, m.L), "@PG\tID:ma_hip\tPN:ma_hip"]
    recs = ref.sorted_records(m)
    assert len(lines) == 4 + len(recs)
    starts = [r["start"] for r in recs]
    assert starts == sorted(starts)                            # SO:coordinate
    for r, ln in zip(recs, lines[3:]):
        f = ln.split("\t")
        cigar, seq = f[5], f[9]
        got = ref.rebuild(ln, m.ref_seq)
        cols, ins, clipped = ref.expected_rebuild(r, m.L)
        where = "%s: record %s" % (name, r["id"])
        assert (got["id"], got["rname"], got["start"]) == (r["id"], m.ref_id, r["start"]), where
        assert (got["rc"], got["dr"], got["seg_b"], got["flag_rest"]) == (1 if r["rc"] else 0, 1 if r["dr"] else 0, r["seg"][:1] == "b", 0), where
        assert (got["score"], got["seg"], got["tr"]) == (r["score"], r["seg"][:1], 1 if r["tr"] else 0), where
        assert got["nm"] == direct_nm(r, m.L, m.ref_seq), where
        if cigar == "*":
            # the one thing a line cannot give back: how many '-' columns a record without a single SEQ character had
            assert seq == "*" and cols.replace("-", "") == "" and ins == [] and clipped == "", where
            continue
        assert ref.query_len(cigar) == len(seq), where
        assert r["start"] + ref.ref_len(cigar) <= m.L, where
        assert (got["columns"], got["ins"], got["clipped"]) == (cols, ins, clipped), where
        assert got["nm_count"] == got["nm"], where
        runs = ref.cigar_runs(cigar)
        assert all(a[1] != b[1] for a, b in zip(runs, runs[1:])) and all(k > 0 for k, _ in runs), where
        assert all(op != "S" for _, op in runs[:-1]), where          # a soft clip is the last run


def test_shapes_hold_what_they_promise():
    m, _ = case("sam:sam_shapes")
    got = {r["id"]: ref.fields(r, m.L, m.ref_seq) for r in m.rec}
    walks = {r["id"]: (r["end"] - r["start"] + 1) + sum(len(s) for p, s in ref.ins_table(r).items() if 0 <= p <= r["end"] - r["start"]) for r in m.rec}
    for w in (1, 63, 64, 65, 127, 128, 129, 600):
        assert walks["walk%d" % w] == w and (w <= 3 or walks["walk%di" % w] == w)
    assert got["run100M"][0] == "100M" and got["run192M"][0] == "192M" and got["ins150"][0] == "50M150I180M"
    assert got["digitsM_D"][0] == "1000M1D5M" and got["digitsMD"][0] == "9M1D10M10D99M99D100M100D900M"
    assert got["digitsI"][0] == "1M9I2M10I2M99I2M100I2M1000I3M"
    assert got["ins_at_0"][0] == "3I30M" and got["ins_by_dash"][0] == "3M2I1D1I4M" and got["ins_by_dash"][2] == 4
    assert got["ins_with_dash"][0] == "5M2I7M1I8M" and got["ins_twice"][0] == "6M1I8M3I6M"
    assert got["ins_over_gaps"][0] == "10M5I10M" and got["ins_outside"][0] == "4M1I6M"
    assert got["only_dashes"] == ("*", "*", 70) and got["no_columns"] == ("*", "*", 0) and got["no_columns_pair"] == ("*", "*", 0)
    assert got["end_L"][0] == "30M1S" and got["end_L_dash"][0] == "29M" and got["end_L_ins"][0] == "27M1I1M4S" and got["end_L_ins_dash"][0] == "27M"
    assert got["end_Lm1"][0] == "64M"
    assert {(r["seg"], r["rc"]) for r in m.rec} >= {("f", 0), ("f", 1), ("b", 0), ("b", 1)} and any(r["dr"] for r in m.rec)
    low, _ = case("sam:sam_lower")
    assert low.ref_seq == m.ref_seq.lower() != m.ref_seq
    assert [ref.fields(r, low.L, low.ref_seq) for r in low.rec] == [ref.fields(r, m.L, m.ref_seq) for r in m.rec]
    assert len(case("sam:sam_257")[0].rec) == 257 and len(case("sam:sam_4097")[0].rec) == 4097 and case("sam:sam_empty")[0].rec == []
    circular = [r for f in ("fix_c.1", "fix_c.2") for r in case("file:" + f)[0].rec if r["end"] >= case("file:" + f)[0].L]
    assert circular, "no committed record ends on column L"


@pytest.mark.parametrize("name", NAMES)
def test_host_build_of_the_kernels_code_agrees(driver, name, tmp_path):
    m, text = case(name)
    path = str(tmp_path / "in.maln")
    with open(path, "w", encoding="latin1") as f:
        f.write(ms.MA_HEADER + text)
    got = subprocess.run([driver, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert got.returncode == 0, got.stderr.decode("latin1")[-2000:]
    want = []
    for r in ref.sorted_records(m):
        b, nm = ref.body(r, m.L, m.ref_seq)
        want.append("%d\t%s\n" % (nm, b))
    want = "".join(want).encode("latin1")
    if got.stdout != want:
        a, b = got.stdout.split(b"\n"), want.split(b"\n")
        at = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        pytest.fail(f"{name}: record {at}: {a[at:at + 1]!r} instead of {b[at:at + 1]!r}")


def test_negative_gap_is_refused_on_the_host(driver, tmp_path):
    bad = sc.negative_gap(case("sam:sam_257")[0])
    path = str(tmp_path / "neg.maln")
    with open(path, "w", encoding="latin1") as f:
        f.write(ms.MA_HEADER + ms.write_maln(bad))
    got = subprocess.run([driver, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert got.returncode == 1 and got.stdout == b""


def test_sam_symbols_declared_and_exported():
    import mia_amd
    hdr = open(os.path.join(ROOT, "include", "mia_hip.h")).read()
    declared = set(re.findall(r"\b(mia_hip_[a-z_0-9]+)\s*\(", hdr))
    lib = mia_amd.lib()
    for sym in ("mia_hip_ma_sam", "mia_hip_get_ma_sam"):
        assert sym in declared, sym
        assert sym in mia_amd.exported_symbols(), sym
        assert hasattr(lib, sym), sym
    assert hasattr(mia_amd.MiaHip, "ma_sam")
    assert {"k_ma_sam_layout", "k_ma_sam_render"} <= set(mia_amd.MiaHip.STAGES)
    assert os.path.exists(os.path.join(ROOT, "mapping-iterative-assembler_amd", "csrc", "ma_sam_body.h"))
