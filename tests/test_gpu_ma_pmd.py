"""The damage score on the GPU: MiaHip.ma_score (mia_hip_ma_score: k_ma_score_cols over the flat columns, k_ma_score_molecules over the
records -- csrc/mia_ma_pmd_kernels.h) must give exactly rec_score, mol_score, keep, hist and the totals of tests/ma_pmd_ref.py, the rule
of DESIGN.md ("Damage score") restated as a loop, for every shape of tests/maln_pmd_cases.py, every use mask, the library's own
double- and single-stranded tables, a random table and the cases' own, at thresholds 0, 3 nat and the case's median score; and ma_hip
-L / -K / -S / -f 97 must print, byte for byte, what the compiled reference's `ma` printed for the files the restatement reduced
(tests/golden/ma_pmd, tools/make_ma_pmd_goldens.py)."""
import ctypes as C
import gzip
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import ma_damage_ref
import ma_dedup_ref
import ma_pmd_ref as ref
import maln_dedup_cases
import maln_pmd_cases as pc
import maln_synth as ms
from conftest import ROOT

pytestmark = pytest.mark.gpu

MA = os.path.join(ROOT, "mapping-iterative-assembler_amd", "ma_hip")
GOLD = os.path.join(ROOT, "tests", "golden", "ma_pmd")
GOLD_IN = os.path.join(ROOT, "tests", "golden", "ma_damage")
ERR_ARG, ERR_STATE = -2, -4                # MIA_HIP_ERR_ARG, MIA_HIP_ERR_STATE (include/mia_hip.h)
STAGES = ("k_ma_score_cols", "k_ma_score_molecules")
OTHER_MODEL = (0.2, 0.02, 0.001, 0.0005)
READ_SETS = ("reads_a", "reads_b")
_ev, _rec, _gold, _sets, _lib_tables = {}, {}, [], {}, {}


@pytest.fixture(scope="module")
def hip():
    import mia_amd
    return mia_amd.MiaHip(0)


def lib_table(ss=False, params=ref.DEFAULTS):
    import mia_amd
    if (ss, params) not in _lib_tables:
        _lib_tables[ss, params] = mia_amd.ma_pmd_table(*params, single_stranded=ss)
    return _lib_tables[ss, params]


def tally(hip, m):
    hip.set_pssm(m.fpsm, m.rpsm)
    hip.ma_tally(*ms.ma_tally_args(ms.flatten(m)))


def wanted(name, which, tag, w):
    """the restatement's record scores of a case under its which-th use mask and a table, made once"""
    if name not in _ev:
        _ev[name] = ref.events(pc.case(name)[0])
    if (name, which, tag) not in _rec:
        _rec[name, which, tag] = ref.record_scores(pc.case(name)[0], w, pc.uses(name)[which], _ev[name])
    return _rec[name, which, tag]


def check(got, want, what):
    for k, field in enumerate(("rec_score", "mol_score", "keep")):
        bad = np.nonzero(got[k] != want[k])[0]
        assert bad.size == 0, (what, field, bad[:5].tolist(), got[k][bad[:5]].tolist(), want[k][bad[:5]].tolist())
    assert np.array_equal(got[3], want[3]), (what, "hist", np.argwhere(got[3] != want[3])[:5].tolist())
    assert got[4:] == want[4:], (what, got[4:], want[4:])


def check_case(hip, name, few=False):
    m, _ = pc.case(name)
    mate = ma_dedup_ref.pair_halves(m.rec)
    tabs = pc.tables(name, lib_table(False), lib_table(True))
    for which, use in enumerate(pc.uses(name)):
        for tag, w in tabs[1:] if few else tabs:
            rec = wanted(name, which, tag, w)
            thresholds = pc.thresholds(name, ref.score(m, w, 0, use, mate, rec)[1])
            for threshold in thresholds[2:] if few else thresholds:
                check(hip.ma_score(m.ref_seq, w, threshold, use, mate), ref.score(m, w, threshold, use, mate, rec),
                      "%s use %d table %s threshold %d" % (name, which, tag, threshold))
    if not (mate != -1).any():                               # no halves: mate may be left out
        check(hip.ma_score(m.ref_seq, lib_table(), 3 * 65536), ref.score(m, lib_table(), 3 * 65536, rec=wanted(name, 0, "ds", lib_table())), name + " without mate")


@pytest.mark.parametrize("name", pc.CASES)
def test_library_call_matches_the_restatement(hip, name):
    tally(hip, pc.case(name)[0])
    check_case(hip, name)


def test_twice_on_one_context_and_behind_another_tally(hip):
    """buffers are reused: large, small, empty, large again; a second call on the same tally; results do not leak between jobs"""
    for name in ("edges", "signs", "empty", "span3", "wrap", "big", "mixed_reversed", "lens"):
        tally(hip, pc.case(name)[0])
        check_case(hip, name, True)
        check_case(hip, name, True)


def test_launch_counts(hip):
    for name in ("signs", "mixed", "empty"):
        m, _ = pc.case(name)
        tally(hip, m)
        hip.stage_stats(reset=True)
        mate = ma_dedup_ref.pair_halves(m.rec)
        for threshold in (-5, 0, 7 * 65536):
            hip.ma_score(m.ref_seq, lib_table(), threshold, None, mate)
        st = hip.stage_stats()
        for stage in STAGES:
            assert st[stage][1] == (3 if m.rec else 0), (name, stage)      # one launch of each per call, none without records


def test_argument_and_state_errors():
    import mia_amd
    hip = mia_amd.MiaHip(0)
    m, _ = pc.case("wrap")
    ref_c = C.c_char_p(m.ref_seq.encode("latin1"))
    mate = ma_dedup_ref.pair_halves(m.rec)
    table = lib_table()
    n1, n2 = C.c_int64(), C.c_int64()

    def call(ref_seq=ref_c, mate=mate, w=table):
        mt = np.ascontiguousarray(mate, np.int64)
        wt = None if w is None else np.ascontiguousarray(w, np.int32)
        return hip._l.mia_hip_ma_score(hip._h, ref_seq, None, mt.ctypes.data_as(C.c_void_p), None if wt is None else wt.ctypes.data_as(C.c_void_p), 3 * 65536,
                                       C.byref(n1), C.byref(n2))

    def getter():
        return hip._l.mia_hip_get_ma_score(hip._h, None, None, None, None, None)

    def changed(a, i, v):
        b = a.copy()
        b[i] = v
        return b

    assert call() == ERR_STATE and getter() == ERR_STATE                                   # no tally yet
    tally(hip, m)
    assert getter() == ERR_STATE                                                         # no call since the tally
    pair = int(np.nonzero(mate >= 0)[0][0])
    whole = int(np.nonzero(mate == -1)[0][0])
    for bad in (dict(ref_seq=None), dict(w=None), dict(w=changed(table, (3, 1, 3), (1 << 20) + 1)), dict(w=changed(table, (30, 4, 4), -(1 << 20) - 1)),
                dict(w=changed(table, (0, 0, 0), -2 ** 31)), dict(mate=changed(mate, whole, len(mate))), dict(mate=changed(mate, whole, -3)),
                dict(mate=changed(mate, whole, whole)), dict(mate=changed(mate, whole, pair))):
        assert call() == 0 and getter() == 0
        assert call(**bad) == ERR_ARG, bad
        assert getter() == ERR_STATE, bad                                                # a refused call leaves no result
    assert call(w=changed(table, (3, 1, 3), 1 << 20)) == 0 and call(w=changed(table, (3, 1, 3), -(1 << 20))) == 0      # the bound itself is fine
    check(hip.ma_score(m.ref_seq, table, 3 * 65536, None, mate), ref.score(m, table, 3 * 65536), "wrap after the refusals")
    assert getter() == 0                                                                 # every pointer may be NULL
    # records tallied with col_off[0] != 0
    f = ms.flatten(m)
    args = list(ms.ma_tally_args(f))
    args[4], args[5], args[6] = f["col_off"] + 16, np.concatenate([np.full(16, 65, np.uint8), f["seq"]]), np.concatenate([np.full(16, 65, np.uint8), f["smp"]])
    hip.ma_tally(*args)
    assert call() == ERR_ARG and getter() == ERR_STATE
    tally(hip, m)
    assert getter() == ERR_STATE and call() == 0 and getter() == 0


# ---- ma_hip ---------------------------------------------------------------------------------------------------------------------------
def write(m, path):
    with open(path, "w", encoding="latin1") as f:
        f.write(ms.MA_HEADER + ms.write_maln(m))
    return path


def ma_hip(path, args):
    return subprocess.run([MA, "-M", path] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


def ok(path, args):
    r = ma_hip(path, args)
    assert r.returncode == 0, (args, r.stderr[-300:])
    return r.stdout


def gold():
    if not _gold:
        with gzip.open(os.path.join(GOLD, "outputs.json.gz")) as f:
            _gold.append(json.load(f))
    return _gold[0]["sets"]


def golden_set(name, tmp_path):
    """(path of the committed file the reference wrote, its Maln)"""
    with gzip.open(os.path.join(GOLD_IN, name + ".maln.1.gz"), "rb") as f:
        data = f.read()
    path = str(tmp_path / (name + ".maln"))
    with open(path, "wb") as g:
        g.write(data)
    if name not in _sets:
        _sets[name] = ms.parse_maln(data.decode("latin1").split("\n", 1)[1])
    return path, _sets[name]


@pytest.mark.parametrize("tag", sorted(gold()[READ_SETS[0]]))
@pytest.mark.parametrize("name", READ_SETS)
def test_ma_hip_L_on_the_references_file_is_the_references_ma_on_the_reduced_file(name, tag, tmp_path):
    path, m = golden_set(name, tmp_path)
    entry = gold()[name][tag]
    nat, lib = tag.split("_")
    for key, args in (("f41c1", ["-f", "41", "-c", "1"]), ("f5", ["-f", "5"])):
        out = ok(path, ["-L", nat] + (["-S"] if lib == "ss" else []) + args)
        want = entry[key]
        if isinstance(want, dict):
            assert (len(out), hashlib.sha256(out).hexdigest()) == (want["bytes"], want["sha256"]), (name, tag, key)
        else:
            assert out == want.encode("latin1"), (name, tag, key)


def test_the_golden_reductions_and_the_file_L_writes(tmp_path):
    for name in READ_SETS:
        assert {"3_ds", "0_ds", "5_ds", "3_ss", "8_ds"} == set(gold()[name])
        cls = gold()[name]["3_ds"]["molecules"]
        assert min(min(c) for c in cls) >= 20                # a filter that kept everything or nothing cannot pass
        assert gold()[name]["3_ds"]["range"][0] < -65536 and gold()[name]["3_ds"]["range"][1] > 21.5 * 65536
    path, m = golden_set("reads_b", tmp_path)
    out = str(tmp_path / "out.maln")
    ok(path, ["-L", "3", "-f", "5", "-m", out])
    assert open(out, "rb").read().split(b"\n", 2)[1] == b"MALN_NAS %d" % gold()["reads_b"]["3_ds"]["kept"]
    assert 0 < gold()["reads_b"]["3_ds"]["kept"] < len(m.rec)
    # -f 97 of the committed file: the library's table on both sides, every molecule in the bin the restatement gives it
    assert ok(path, ["-f", "97", "-A"]).decode() == ref.table(m, lib_table(), True)


@pytest.mark.parametrize("name", ("signs", "wrap", "mixed", "big"))
def test_L_is_the_restatements_reduced_file(name, tmp_path):
    m, _ = pc.case(name)
    path = write(m, str(tmp_path / "in.maln"))
    for nat, ss in (("3", False), ("3", True), ("-0.5", False)):
        w = lib_table(ss)
        keep = ref.score(m, w, ref.threshold_of(float(nat)))[2]
        less = ref.reduce(m, keep)
        lib_args = ["-S"] if ss else []
        out = str(tmp_path / "out.maln")
        assert ok(path, ["-L", nat] + lib_args + ["-f", "97", "-A", "-m", out]).decode() == ref.table(less, w, True, ss), (name, nat, ss)
        assert open(out, "rb").read().split(b"\n", 2)[1] == b"MALN_NAS %d" % int(keep.sum())
        if not ss:
            assert ok(out, ["-f", "41"]) == ok(write(less, str(tmp_path / "less.maln")), ["-f", "41"]), (name, nat)


@pytest.mark.parametrize("name", ("signs", "wrap", "mixed", "empty"))
def test_f97_is_the_restatements_table(name, tmp_path):
    m, _ = pc.case(name)
    path = write(m, str(tmp_path / "in.maln"))
    k_arg = ",".join("%g" % x for x in OTHER_MODEL)
    for use_dropped in (False, True):
        for ss in (False, True):
            args = ["-f", "97"] + (["-A"] if use_dropped else []) + (["-S"] if ss else [])
            assert ok(path, args).decode() == ref.table(m, lib_table(ss), use_dropped, ss), args
            if use_dropped != ss:
                out = ok(path, args + ["-K", k_arg]).decode()
                assert out == ref.table(m, lib_table(ss, OTHER_MODEL), use_dropped, ss, OTHER_MODEL), args
                assert out.split("\n")[0].endswith("library %s, p 0.2 c0 0.02 pi 0.001 eps 0.0005" % ("ss" if ss else "ds"))
    assert ok(path, ["-f", "97", "-I", "other", "-c", "2"]).decode() == ref.table(m, lib_table())        # -I and -c have no effect
    if name != "empty":
        w = lib_table(False, OTHER_MODEL)
        keep = ref.score(m, w, ref.threshold_of(1.5))[2]
        assert ok(path, ["-L", "1.5", "-K", k_arg, "-f", "97"]).decode() == ref.table(ref.reduce(m, keep), w, False, False, OTHER_MODEL)


def test_u_D_L_E_m_compose(tmp_path):
    """-u, -D, then -L, then -E: each step on the file the step before wrote"""
    path, m = golden_set("reads_a", tmp_path)
    u, d, l, e, all_out = (str(tmp_path / x) for x in ("u.maln", "d.maln", "l.maln", "e.maln", "out.maln"))
    ok(path, ["-u", "-f", "5", "-m", u])
    ok(u, ["-D", "3", "-f", "5", "-m", d])
    ok(d, ["-L", "0", "-f", "5", "-m", l])
    direct = ok(path, ["-u", "-D", "3", "-L", "0", "-E", "3", "-m", all_out])
    assert direct == ok(l, ["-E", "3", "-m", e]) and direct.startswith(b"CLUSTAL W") and len(direct) > 500

    def body(fn):                                            # (line 1 carries the date)
        return open(fn, "rb").read().split(b"\n", 1)[1]

    assert body(all_out) == body(e) and 0 < int(body(e).split(b"\n", 1)[0][9:]) < len(m.rec)
    # a threshold that bites behind -D 3 (a hit within three positions is worth more than 3 nat): fewer records than without -L
    ok(path, ["-u", "-D", "3", "-L", "8", "-f", "97", "-m", all_out])
    assert 0 < int(body(all_out).split(b"\n", 1)[0][9:]) < int(body(d).split(b"\n", 1)[0][9:])


def test_option_errors(tmp_path):
    path = write(pc.case("signs")[0], str(tmp_path / "in.maln"))
    for args, words in ((["-K", "0.3,0.01,0.001,0.001", "-f", "41"], (b"-K", b"-L", b"97")), (["-K", "0.3,0.01,0.001,0.001"], (b"-K", b"-L", b"97")),
                        (["-L", "x"], (b"-L",)), (["-L", ""], (b"-L",)), (["-L", "3x"], (b"-L",)), (["-L", "nan"], (b"-L",)), (["-L", "inf"], (b"-L",)),
                        (["-L", "1e300"], (b"-L",)), (["-L", "3", "-K", "0.3,0.01,0.001"], (b"-K",)), (["-L", "3", "-K", "0.3,0.01,0.001,0.001,0.5"], (b"-K",)),
                        (["-L", "3", "-K", "0.3;0.01;0.001;0.001"], (b"-K",)), (["-L", "3", "-K", "a,b,c,d"], (b"-K",)), (["-f", "97", "-K", ""], (b"-K",)),
                        (["-L", "3", "-K", "1,0.01,0.001,0.001"], (b"-K",)), (["-L", "3", "-K", "0.3,0.8,0.001,0.001"], (b"-K",)),
                        (["-f", "97", "-K", "0.3,0.01,0,0.001"], (b"-K",)), (["-f", "97", "-K", "0.3,0.01,0.001,nan"], (b"-K",)),
                        (["-f", "97", "-K", "0.3,0.01,1e-12,1e-12"], (b"-K",)), (["-S", "-f", "41"], (b"-S", b"-D")), (["-E", "3", "-f", "97"], (b"-E", b"97"))):
        r = ma_hip(path, args)
        assert r.returncode == 1 and r.stdout == b"" and len(r.stderr.strip().split(b"\n")) == 1, (args, r.stderr)
        assert all(w in r.stderr for w in words), (args, r.stderr)
    assert ok(path, ["-S", "-f", "97"]).startswith(b"# ma_hip damage scores")                       # -S with -f 97 or -L alone is fine
    assert len(ok(path, ["-S", "-L", "0", "-f", "41"])) > 100
    for fmt in ("3", "94"):
        r = ma_hip(path, ["-f", fmt])
        assert r.returncode != 0 and b"outside the MI355X-accelerated path" in r.stderr and b"97" in r.stderr and r.stdout == b""
    r = subprocess.run([MA], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0 and all(w in r.stdout for w in (b"-L", b"-K", b"97"))


def test_the_run_without_the_new_options_is_unchanged(tmp_path):
    """-f 41 against the reference's recorded output (tests/golden/ma_synth), -u -f 41 and -D 3 -f 41 against the reference's recorded
    outputs for the files the other filters' restatements reduced (tests/golden/ma_dedup, tests/golden/ma_damage), -f 95 -- a report
    the reference does not have -- against tests/ma_damage_ref.py"""
    from test_ma_synth_cpu import case, recorded
    for name in ("edge256", "codes_anc"):
        m, _ = case(name)
        path = write(m, str(tmp_path / (name + ".maln")))
        assert ok(path, ["-f", "41", "-c", "1"]) == recorded(name, "f41c1")[0].encode("latin1"), name
    with gzip.open(os.path.join(ROOT, "tests", "golden", "ma_dedup", "outputs.json.gz")) as f:
        dedup = json.load(f)["cases"]
    for name in ("hand", "wrap"):
        path = write(maln_dedup_cases.case(name), str(tmp_path / (name + ".maln")))
        assert ok(path, ["-u", "-f", "41", "-c", "1"]) == dedup[name]["0"]["f41c1"].encode("latin1"), name
    with gzip.open(os.path.join(GOLD_IN, "outputs.json.gz")) as f:
        damage = json.load(f)["sets"]
    path, m = golden_set("reads_a", tmp_path)
    assert ok(path, ["-D", "3", "-f", "41", "-c", "1"]) == damage["reads_a"]["3_any_ds"]["f41c1"].encode("latin1")
    assert ok(path, ["-f", "95"]).decode() == ma_damage_ref.table(m)
