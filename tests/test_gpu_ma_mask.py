"""The end mask on the GPU: MiaHip.ma_mask (mia_hip_ma_mask: k_ma_mask_bounds over the flat columns, k_ma_mask_layout over the records,
k_ma_mask_apply over the new layout and the pairs -- csrc/mia_ma_mask_kernels.h) must give exactly the arrays and counts of
tests/ma_mask_ref.py, the rule of DESIGN.md ("End mask") restated as a loop, for the committed reference-written files, for maln_synth's
codes_anc and deep and for every shape of tests/maln_mask_cases.py; and ma_hip -E / -x / -S / -f 96 must print, byte for byte, what the
compiled reference's `ma` printed for the files the restatement masked (tests/golden/ma_mask, tools/make_ma_mask_goldens.py)."""
import copy
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
import ma_mask_goldens as mg
import ma_mask_ref as ref
import maln_mask_cases as kc
import maln_synth as ms
from conftest import ROOT

pytestmark = pytest.mark.gpu

MA = os.path.join(ROOT, "mapping-iterative-assembler_amd", "ma_hip")
ERR_ARG, ERR_STATE = -2, -4                # MIA_HIP_ERR_ARG, MIA_HIP_ERR_STATE (include/mia_hip.h)
STAGES = ("k_ma_mask_bounds", "k_ma_mask_layout", "k_ma_mask_apply")
MORE = ((15, 1, False, False), (1, 15, True, True))
_gold, _synth = [], {}


@pytest.fixture(scope="module")
def hip():
    import mia_amd
    return mia_amd.MiaHip(0)


def tally(hip, m):
    hip.set_pssm(m.fpsm, m.rpsm)
    hip.ma_tally(*ms.ma_tally_args(ms.flatten(m)))


def synth(name):
    if name not in _synth:
        _synth[name] = ms.make_case(name)
    return _synth[name]


def check(got, want, what):
    for key in ("first", "count", "start", "col_off", "pair_keep", "ins_pos"):
        a, b = got[key], getattr(want, key)
        assert a.shape == b.shape, (what, key, a.shape, b.shape)
        bad = np.nonzero(a != b)[0]
        assert bad.size == 0, (what, key, bad[:5].tolist(), a[bad[:5]].tolist(), b[bad[:5]].tolist())
    for key in ("seq", "smp"):
        a, b = got[key], np.frombuffer(getattr(want, key), np.uint8)
        assert a.shape == b.shape, (what, key, a.shape, b.shape)
        bad = np.nonzero(a != b)[0]
        assert bad.size == 0, (what, key, bad[:5].tolist(), a[bad[:5]].tolist(), b[bad[:5]].tolist())
    assert np.array_equal(got["hist"], want.hist), (what, "hist", np.argwhere(got["hist"] != want.hist)[:5].tolist())
    c = want.counts()
    for key in ("emptied", "stripped", "pairs_dropped", "n_kept", "cols_kept"):
        assert got[key] == c[key], (what, key, got[key], c[key])


def check_all(hip, m, name, settings=ref.SETTINGS + MORE):
    tally(hip, m)
    for s in settings:
        check(hip.ma_mask(*s), ref.mask(m, *s), (name,) + s)


@pytest.mark.parametrize("name", kc.CASES)
def test_edge_shapes_match_the_restatement(hip, name):
    check_all(hip, kc.case(name), name)


@pytest.mark.parametrize("name", sorted(mg.INPUTS))
def test_golden_inputs_match_the_restatement(hip, name):
    check_all(hip, mg.load(name), name)


def test_codes_anc_matches_the_restatement(hip):
    check_all(hip, synth("codes_anc"), "codes_anc")


def test_deep_matches_the_restatement(hip):
    """20 000 records, 2.87 M columns: more chunks than the persistent grid has workgroups, 79 workgroups in the ordered scan"""
    check_all(hip, synth("deep"), "deep", ((15, 15, False, False), (3, 2, False, False), (3, 3, True, False)))


@pytest.mark.parametrize("name", ("offsets", "codes", "dashes", "chunk_edge"))
def test_the_result_does_not_depend_on_the_records_order(hip, name):
    m = kc.case(name)
    perm = ms.Rng(96).permutation(len(m.rec)).tolist()
    moved = ms.Maln()
    moved.L, moved.ref_seq, moved.gaps, moved.fpsm, moved.rpsm = m.L, m.ref_seq, m.gaps, m.fpsm, m.rpsm
    moved.rec = [m.rec[p] for p in perm]
    tally(hip, moved)
    pair_at = {}                                             # (record, pair of the record) -> pair number
    for mm, key in ((m, "a"), (moved, "b")):
        e = 0
        for r, rec in enumerate(mm.rec):
            for k in range(len(rec["ins"])):
                pair_at[key, r, k] = e
                e += 1
    for s in ((3, 3, False, False), (15, 15, False, False), (3, 3, True, False)):
        got, want = hip.ma_mask(*s), ref.mask(m, *s)
        check(got, ref.mask(moved, *s), (name, "moved") + s)
        for key in ("first", "count", "start"):              # un-shuffled: record perm[i] of the original is record i of the moved file
            assert np.array_equal(got[key], getattr(want, key)[perm]), (name, key, s)
        for i, p in enumerate(perm):
            a, b = int(want.col_off[p]), int(got["col_off"][i])
            n = int(want.count[p])
            assert bytes(got["seq"][b:b + n]) == want.seq[a:a + n] and bytes(got["smp"][b:b + n]) == want.smp[a:a + n], (name, s, p)
            for k in range(len(m.rec[p]["ins"])):
                ea, eb = pair_at["a", p, k], pair_at["b", i, k]
                assert (got["pair_keep"][eb], got["ins_pos"][eb]) == (want.pair_keep[ea], want.ins_pos[ea]), (name, s, p, k)
        assert np.array_equal(got["hist"], want.hist)
        assert [got[k] for k in ("emptied", "stripped", "pairs_dropped", "n_kept", "cols_kept")] == [want.counts()[k] for k in ("emptied", "stripped", "pairs_dropped", "n_kept", "cols_kept")]


def test_twice_on_one_context_and_behind_another_tally(hip):
    """buffers are reused: large, small, empty, large again; results do not leak between jobs or between modes"""
    few = ((3, 3, False, False), (3, 3, True, True), (15, 15, False, False))
    for name in ("codes", "one_col", "empty", "long_5000", "all_emptied", "pairs300"):
        check_all(hip, kc.case(name), name, few)
        check_all(hip, kc.case(name), name, few[::-1])


def test_launch_counts(hip):
    for name in ("dashes", "codes", "empty"):
        m = kc.case(name)
        tally(hip, m)
        hip.stage_stats(reset=True)
        for s in ((3, 3, False, False), (15, 0, False, False), (3, 3, True, False)):
            hip.ma_mask(*s)
        st = hip.stage_stats()
        for stage in STAGES:
            assert st[stage][1] == (3 if m.rec else 0), (name, stage)      # one launch of each per call, none without records


def test_argument_and_state_errors():
    import mia_amd
    hip = mia_amd.MiaHip(0)
    m = kc.case("dashes")
    n1, n2 = C.c_int64(), C.c_int64()

    def call(n5=3, n3=3, mode=0, ss=0):
        return hip._l.mia_hip_ma_mask(hip._h, n5, n3, mode, ss, C.byref(n1), C.byref(n2))

    def getter():
        return hip._l.mia_hip_get_ma_mask(hip._h, None, None, None, None, None, None, 0, None, None, None, None)

    assert call() == ERR_STATE and getter() == ERR_STATE                                   # no tally yet
    tally(hip, m)
    assert getter() == ERR_STATE                                                         # no call since the tally
    for bad in (dict(n5=0, n3=0), dict(n5=16), dict(n3=16), dict(n5=-1), dict(n3=-1), dict(mode=2), dict(mode=-1), dict(ss=1), dict(mode=0, ss=1)):
        assert call() == 0 and getter() == 0
        assert call(**bad) == ERR_ARG, bad
        assert getter() == ERR_STATE, bad                                                # a refused call leaves no result
    assert call(mode=1, ss=1) == 0 and call(n5=0, n3=15) == 0 and call(n5=15, n3=0) == 0
    check(hip.ma_mask(3, 3), ref.mask(m, 3, 3), "dashes after the refusals")
    assert getter() == 0                                                                 # every pointer may be NULL
    seq = np.zeros(4, np.uint8)                                                          # a buffer that is too small
    assert hip._l.mia_hip_get_ma_mask(hip._h, None, None, None, None, seq.ctypes.data_as(C.c_void_p), None, 4, None, None, None, None) == ERR_ARG
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
        with gzip.open(os.path.join(ROOT, "tests", "golden", "ma_mask", "outputs.json.gz")) as f:
            _gold.append(json.load(f))
    return _gold[0]["files"]


def golden_file(name, tmp_path):
    path = str(tmp_path / (name + ".maln"))
    with open(path, "w", encoding="latin1") as f:
        f.write(mg.text(name))
    return path


@pytest.mark.parametrize("setting", ref.SETTINGS, ids=[ref.tag(*s) for s in ref.SETTINGS])
@pytest.mark.parametrize("name", sorted(mg.INPUTS))
def test_ma_hip_E_on_the_references_file_is_the_references_ma_on_the_masked_file(name, setting, tmp_path):
    path = golden_file(name, tmp_path)
    entry = gold()[name][ref.tag(*setting)]
    for key, args in mg.RUNS:
        out = ok(path, mg.e_args(*setting) + args)
        want = entry[key]
        if isinstance(want, dict):
            assert (len(out), hashlib.sha256(out).hexdigest()) == (want["bytes"], want["sha256"]), (name, setting, key)
        else:
            assert out == want.encode("latin1"), (name, setting, key)
    assert ok(path, mg.e_args(*setting) + ["-f", "96"]).decode() == ref.report_of(len(mg.load(name).rec), entry["counts"], setting[2], setting[3])


def test_one_number_means_both_ends(tmp_path):
    path = golden_file("fix_c_anc", tmp_path)
    assert ok(path, ["-E", "3", "-f", "41"]) == ok(path, ["-E", "3,3", "-f", "41"]) != ok(path, ["-E", "3,0", "-f", "41"])
    assert ok(path, ["-E", "3", "-f", "41"]) != ok(path, ["-f", "41"])


def test_u_then_D_then_E_is_the_restatements_in_that_order(tmp_path):
    """the damaged reads the reference assembled (tests/golden/ma_damage), every second record given twice: each of the three steps
    takes something"""
    src = mg.load("reads_a")
    m = copy.copy(src)
    m.rec = sorted(list(src.rec) + [dict(r, id="dup" + r["id"], score=r["score"] - 1) for r in src.rec[::2]], key=lambda r: (r["start"], r["end"]))
    path, n_file = write(m, str(tmp_path / "in.maln")), len(m.rec)
    unique = ma_dedup_ref.reduce(m, ma_dedup_ref.dedup(m.rec, m.L)[0])
    m = ma_damage_ref.reduce(unique, ma_damage_ref.damage(unique, 3)[2])
    got = ref.mask(m, 3, 3)
    assert n_file > len(unique.rec) > len(m.rec) > 0 and len(got.maln.rec) > 0 and got.hist.sum() > 0
    want = ms.restate(got.maln)
    assert ok(path, ["-u", "-D", "3", "-E", "3", "-f", "41", "-c", "1"]).decode("latin1") == want.table(1)
    assert ok(path, ["-u", "-D", "3", "-E", "3", "-f", "5"]).decode("latin1") == want.f5(1)
    assert ok(path, ["-u", "-D", "3", "-E", "3", "-f", "96"]).decode() == ref.report_of(len(m.rec), got.counts(), False, False)
    m_ss = ma_damage_ref.reduce(unique, ma_damage_ref.damage(unique, 3, ss=True)[2])       # -S is the library of -D and of -x alike
    assert ok(path, ["-u", "-D", "3", "-S", "-E", "3", "-x", "-f", "96"]).decode() == ref.report(m_ss, 3, 3, True, True)


def same_file(a, b):
    """two Malns as -m writes them: NUM_INPUTS and DR are always written, pairs in ascending position, of one position the last"""
    assert (a.L, a.ref_seq, a.ref_id, len(a.rec)) == (b.L, b.ref_seq, b.ref_id, len(b.rec))
    assert np.array_equal(a.gaps, b.gaps), np.nonzero(a.gaps != b.gaps)[0][:5].tolist()
    for x, y in zip(a.rec, b.rec):
        last = {}
        for p, s in y["ins"]:
            if 0 <= p < len(y["seq"]):
                last[p] = s
        want = dict(y, ins=sorted(last.items()), num_inputs=y["num_inputs"] if y["num_inputs"] is not None else 1, dr=y["dr"] or 0)
        assert x == want, (x["id"], {k: (x[k], want[k]) for k in x if x[k] != want[k]})


@pytest.mark.parametrize("name", ("offsets", "dashes", "pairs300", "all_emptied"))
def test_m_writes_the_restatements_file(name, tmp_path):
    m = kc.case(name)
    srt = ms.Maln()
    srt.__dict__.update(m.__dict__)
    srt.rec = sorted(m.rec, key=lambda r: (r["start"], r["end"]))                         # ma sorts before it masks and writes (a stable sort)
    path = write(m, str(tmp_path / "in.maln"))
    for s in ((3, 3, False, False), (15, 15, False, False), (3, 3, True, True)):
        out = str(tmp_path / "out.maln")
        ok(path, mg.e_args(*s) + ["-f", "5", "-m", out])
        with open(out, encoding="latin1") as f:
            got = ms.parse_maln(f.read().split("\n", 1)[1])
        want = ref.mask(srt, *s).maln
        want.rec = sorted(want.rec, key=lambda r: (r["start"], r["end"]))
        same_file(got, want)
        if got.rec:
            assert ok(out, ["-f", "41"]) == ok(path, mg.e_args(*s) + ["-f", "41"])


@pytest.mark.parametrize("name", ("dashes", "codes", "empty", "all_emptied"))
def test_f96_is_the_restatements_report(name, tmp_path):
    m = kc.case(name)
    path = write(m, str(tmp_path / "in.maln"))
    for s in ((3, 3, False, False), (15, 15, False, False), (0, 7, False, False), (3, 3, True, False), (15, 15, True, True)):
        assert ok(path, mg.e_args(*s) + ["-f", "96"]).decode() == ref.report(m, *s), s
    assert ok(path, ["-E", "3", "-f", "96", "-I", "other", "-c", "2"]).decode() == ref.report(m, 3, 3)          # -I and -c have no effect


def test_option_errors(tmp_path):
    path = write(kc.case("dashes"), str(tmp_path / "in.maln"))
    for args, words in ((["-E", "3", "-f", "92"], (b"-E", b"92")), (["-E", "3", "-f", "93"], (b"-E", b"93")), (["-E", "3", "-f", "95"], (b"-E", b"95")),
                        (["-x", "-f", "41"], (b"-x", b"-E")), (["-f", "96"], (b"96", b"-E")), (["-E", "0"], (b"-E",)), (["-E", "0,0"], (b"-E",)),
                        (["-E", "16"], (b"-E",)), (["-E", "3,16"], (b"-E",)), (["-E", "-1"], (b"-E",)), (["-E", "3,"], (b"-E",)), (["-E", ",3"], (b"-E",)),
                        (["-E", "3,3,3"], (b"-E",)), (["-E", "2.5"], (b"-E",)), (["-E", "x"], (b"-E",)), (["-E", "3", "-S"], (b"-S",))):
        r = ma_hip(path, args)
        assert r.returncode == 1 and r.stdout == b"" and len(r.stderr.strip().split(b"\n")) == 1, (args, r.stderr)
        assert all(w in r.stderr for w in words), (args, r.stderr)
    for fmt in ("3", "94"):
        r = ma_hip(path, ["-E", "3", "-f", fmt])
        assert r.returncode != 0 and b"outside the MI355X-accelerated path" in r.stderr and b"96" in r.stderr and r.stdout == b""
    r = subprocess.run([MA], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0 and all(w in r.stdout for w in (b"-E", b"-x", b"96"))


def test_the_run_without_the_new_options_is_unchanged(tmp_path):
    """-f 41 against the reference's recorded output (tests/golden/ma_synth), -D against the reference's recorded output for the file the
    deaminated-fragment filter's restatement reduced (tests/golden/ma_damage)"""
    from test_ma_synth_cpu import case, recorded
    for name in ("edge256", "codes_anc"):
        m, _ = case(name)
        path = write(m, str(tmp_path / (name + ".maln")))
        assert ok(path, ["-f", "41", "-c", "1"]) == recorded(name, "f41c1")[0].encode("latin1"), name
    with gzip.open(os.path.join(ROOT, "tests", "golden", "ma_damage", "outputs.json.gz")) as f:
        damage = json.load(f)["sets"]
    path = golden_file("reads_a", tmp_path)
    for tag, args in (("3_any_ds", ["-D", "3"]), ("3_3_ss", ["-D", "3", "-e", "3", "-S"])):
        assert ok(path, args + ["-f", "41", "-c", "1"]) == damage["reads_a"][tag]["f41c1"].encode("latin1"), tag
        assert ok(path, args + ["-f", "5"]) == damage["reads_a"][tag]["f5"].encode("latin1"), tag
