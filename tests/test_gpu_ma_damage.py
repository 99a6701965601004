"""The deaminated-fragment filter on the GPU: MiaHip.ma_damage (mia_hip_ma_damage: k_ma_damage_hits over the flat columns,
k_ma_damage_molecules over the records -- csrc/mia_ma_damage_kernels.h) must give exactly pos5, pos3, keep, hist and the totals of
tests/ma_damage_ref.py, the rule of DESIGN.md ("Deaminated fragments") restated as a loop, for every shape of
tests/maln_damage_cases.py, every use mask, both libraries, N in 1, 2, 3, 15 and the four ends modes; and ma_hip -D / -e / -S / -f 95
must print, byte for byte, what the compiled reference's `ma` printed for the files the restatement reduced
(tests/golden/ma_damage, tools/make_ma_damage_goldens.py)."""
import ctypes as C
import gzip
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import ma_damage_ref as ref
import ma_dedup_ref
import ma_profile_ref
import maln_damage_cases as dc
import maln_dedup_cases
import maln_synth as ms
from conftest import ROOT

pytestmark = pytest.mark.gpu

MA = os.path.join(ROOT, "mapping-iterative-assembler_amd", "ma_hip")
GOLD = os.path.join(ROOT, "tests", "golden", "ma_damage")
ERR_ARG, ERR_STATE = -2, -4                # MIA_HIP_ERR_ARG, MIA_HIP_ERR_STATE (include/mia_hip.h)
STAGES = ("k_ma_damage_hits", "k_ma_damage_molecules")
_pos, _gold, _sets = {}, [], {}


@pytest.fixture(scope="module")
def hip():
    import mia_amd
    return mia_amd.MiaHip(0)


def tally(hip, m):
    hip.set_pssm(m.fpsm, m.rpsm)
    hip.ma_tally(*ms.ma_tally_args(ms.flatten(m)))


def wanted(name, which, ss):
    """the restatement's positions of a case under its which-th use mask, made once"""
    if (name, which, ss) not in _pos:
        _pos[name, which, ss] = ref.positions(dc.case(name)[0], dc.uses(name)[which], ss)
    return _pos[name, which, ss]


def check(got, want, what):
    for k, field in enumerate(("pos5", "pos3", "keep")):
        bad = np.nonzero(got[k] != want[k])[0]
        assert bad.size == 0, (what, field, bad[:5].tolist(), got[k][bad[:5]].tolist(), want[k][bad[:5]].tolist())
    assert np.array_equal(got[3], want[3]), (what, "hist", np.argwhere(got[3] != want[3])[:5].tolist())
    assert got[4:] == want[4:], (what, got[4:], want[4:])


def check_case(hip, name, grid=None):
    m, _ = dc.case(name)
    mate = ma_dedup_ref.pair_halves(m.rec)
    for which, use in enumerate(dc.uses(name)):
        for ss in (False, True):
            pos = wanted(name, which, ss)
            for n_pos in ref.GRID_N:
                for mode in ref.MODES:
                    if grid is not None and (n_pos, mode, ss) not in grid:
                        continue
                    check(hip.ma_damage(m.ref_seq, n_pos, use, mate, ss, mode), ref.damage(m, n_pos, mode, ss, use, mate, pos),
                          "%s use %d N=%d %s %s" % (name, which, n_pos, mode, "ss" if ss else "ds"))
    if not (mate != -1).any():                               # no halves: mate may be left out
        check(hip.ma_damage(m.ref_seq, 3), ref.damage(m, 3, pos=wanted(name, 0, False)), name + " without mate")


@pytest.mark.parametrize("name", dc.CASES)
def test_library_call_matches_the_restatement(hip, name):
    tally(hip, dc.case(name)[0])
    check_case(hip, name)


def test_twice_on_one_context_and_behind_another_tally(hip):
    """buffers are reused: large, small, empty, large again; a second call on the same tally; results do not leak between jobs"""
    few = {(1, "any", False), (3, "both", False), (2, "3", True)}
    for name in ("mixed", "hand", "empty", "pile_3000", "wrap", "mixed_reversed", "lens"):
        tally(hip, dc.case(name)[0])
        check_case(hip, name, few)
        check_case(hip, name, few)


def test_launch_counts(hip):
    for name in ("hand", "mixed", "empty"):
        m, _ = dc.case(name)
        tally(hip, m)
        hip.stage_stats(reset=True)
        mate = ma_dedup_ref.pair_halves(m.rec)
        for n_pos in (1, 7, 15):
            hip.ma_damage(m.ref_seq, n_pos, None, mate)
        st = hip.stage_stats()
        for stage in STAGES:
            assert st[stage][1] == (3 if m.rec else 0), (name, stage)      # one launch of each per call, none without records


def test_argument_and_state_errors():
    import mia_amd
    hip = mia_amd.MiaHip(0)
    m, _ = dc.case("wrap")
    ref_c = C.c_char_p(m.ref_seq.encode("latin1"))
    mate = ma_dedup_ref.pair_halves(m.rec)
    n1, n2 = C.c_int64(), C.c_int64()

    def call(ref_seq=ref_c, mate=mate, n_pos=3, mode=0):
        mt = np.ascontiguousarray(mate, np.int64)
        return hip._l.mia_hip_ma_damage(hip._h, ref_seq, None, mt.ctypes.data_as(C.c_void_p), n_pos, 0, mode, C.byref(n1), C.byref(n2))

    def getter():
        return hip._l.mia_hip_get_ma_damage(hip._h, None, None, None, None, None)

    def changed(a, i, v):
        b = a.copy()
        b[i] = v
        return b

    assert call() == ERR_STATE and getter() == ERR_STATE                                   # no tally yet
    tally(hip, m)
    assert getter() == ERR_STATE                                                         # no call since the tally
    pair = int(np.nonzero(mate >= 0)[0][0])
    whole = int(np.nonzero(mate == -1)[0][0])
    for bad in (dict(ref_seq=None), dict(n_pos=0), dict(n_pos=16), dict(n_pos=-1), dict(mode=4), dict(mode=-1), dict(mate=changed(mate, whole, len(mate))),
                dict(mate=changed(mate, whole, -3)), dict(mate=changed(mate, whole, whole)), dict(mate=changed(mate, whole, pair))):
        assert call() == 0 and getter() == 0
        assert call(**bad) == ERR_ARG, bad
        assert getter() == ERR_STATE, bad                                                # a refused call leaves no result
    check(hip.ma_damage(m.ref_seq, 3, None, mate), ref.damage(m, 3), "wrap after the refusals")
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
    with gzip.open(os.path.join(GOLD, name + ".maln.1.gz"), "rb") as f:
        data = f.read()
    path = str(tmp_path / (name + ".maln"))
    with open(path, "wb") as g:
        g.write(data)
    if name not in _sets:
        _sets[name] = ms.parse_maln(data.decode("latin1").split("\n", 1)[1])
    return path, _sets[name]


def d_args(n_pos, mode, ss):
    return ["-D", str(n_pos)] + (["-e", mode] if mode != "any" else []) + (["-S"] if ss else [])


@pytest.mark.parametrize("tag", sorted(gold()[dc.READ_SETS[0]]))
@pytest.mark.parametrize("name", dc.READ_SETS)
def test_ma_hip_D_on_the_references_file_is_the_references_ma_on_the_reduced_file(name, tag, tmp_path):
    path, m = golden_set(name, tmp_path)
    entry = gold()[name][tag]
    n_pos, mode, lib = tag.split("_")
    for key, args in (("f41c1", ["-f", "41", "-c", "1"]), ("f5", ["-f", "5"])):
        out = ok(path, d_args(int(n_pos), mode, lib == "ss") + args)
        want = entry[key]
        if isinstance(want, dict):
            assert (len(out), hashlib.sha256(out).hexdigest()) == (want["bytes"], want["sha256"]), (name, tag, key)
        else:
            assert out == want.encode("latin1"), (name, tag, key)


def test_the_golden_reductions_and_the_file_D_writes(tmp_path):
    for name in dc.READ_SETS:
        assert {"3_any_ds", "1_5_ds", "2_both_ds", "3_3_ss"} <= set(gold()[name])
    path, m = golden_set("reads_b", tmp_path)
    out = str(tmp_path / "out.maln")
    ok(path, ["-D", "3", "-e", "any", "-f", "5", "-m", out])
    assert open(out, "rb").read().split(b"\n", 2)[1] == b"MALN_NAS %d" % gold()["reads_b"]["3_any_ds"]["kept"]
    assert 0 < gold()["reads_b"]["3_any_ds"]["kept"] < len(m.rec)


def test_D_then_m_then_read_again(tmp_path):
    path, _ = golden_set("reads_a", tmp_path)
    out = str(tmp_path / "out.maln")
    direct = ok(path, ["-D", "3", "-f", "41", "-m", out])
    assert ok(out, ["-f", "41"]) == direct and len(direct) > 1000
    assert ok(path, ["-f", "41"]) != direct


@pytest.mark.parametrize("name", ("reads_a", "reads_b"))
def test_u_then_D_is_D_on_the_file_u_wrote(name, tmp_path):
    """the pairing works on the records that are left, whatever their file numbers were (the committed files of the duplicate filter
    hold duplicates and split reads)"""
    with gzip.open(os.path.join(ROOT, "tests", "golden", "ma_dedup", name + ".maln.1.gz"), "rb") as f, open(str(tmp_path / "in.maln"), "wb") as g:
        g.write(f.read())
    path, out = str(tmp_path / "in.maln"), str(tmp_path / "u.maln")
    ok(path, ["-u", "-f", "5", "-m", out])
    for extra in (["-f", "41"], ["-f", "95"], ["-e", "5", "-f", "8"]):
        assert ok(path, ["-u", "-D", "15"] + extra) == ok(out, ["-D", "15"] + extra), extra
    assert ok(path, ["-u", "-D", "15", "-f", "41"]) != ok(path, ["-u", "-f", "41"])


@pytest.mark.parametrize("name", ("hand", "wrap", "mixed", "empty"))
def test_f95_is_the_restatements_table(name, tmp_path):
    m, _ = dc.case(name)
    path = write(m, str(tmp_path / "in.maln"))
    for use_dropped in (False, True):
        for ss in (False, True):
            args = ["-f", "95"] + (["-A"] if use_dropped else []) + (["-S"] if ss else [])
            assert ok(path, args).decode() == ref.table(m, use_dropped, ss), args
    assert ok(path, ["-f", "95", "-I", "other", "-c", "2"]).decode() == ref.table(m)                 # -I and -c have no effect
    if name != "empty":
        keep = ref.damage(m, 3, "5")[2]
        assert ok(path, ["-D", "3", "-e", "5", "-f", "95", "-A"]).decode() == ref.table(ref.reduce(m, keep), True)
        out = str(tmp_path / "out.maln")
        assert ok(path, ["-D", "3", "-e", "5", "-f", "95", "-m", out]).decode() == ref.table(ref.reduce(m, keep))
        assert open(out, "rb").read().split(b"\n", 2)[1] == b"MALN_NAS %d" % int(keep.sum())


def test_conditional_substitution_profile(tmp_path):
    """-D 1 -e 3 -f 9: the profile of the fragments that are deaminated at their 3' end"""
    for name in ("mixed", "wrap"):
        m, _ = dc.case(name)
        keep = ref.damage(m, 1, "3")[2]
        assert 0 < keep.sum() < len(keep)
        less = ref.reduce(m, keep)
        assert ok(write(m, str(tmp_path / "in.maln")), ["-D", "1", "-e", "3", "-f", "9"]).decode() == ma_profile_ref.table(less), name


def test_option_errors(tmp_path):
    path = write(dc.case("hand")[0], str(tmp_path / "in.maln"))
    for args, words in ((["-e", "5", "-f", "41"], (b"-e", b"-D")), (["-S", "-f", "41"], (b"-S", b"-D")), (["-S"], (b"-S", b"-D")),
                        (["-D", "0"], (b"-D",)), (["-D", "16"], (b"-D",)), (["-D", "-1"], (b"-D",)), (["-D", "2.5"], (b"-D",)), (["-D", "x"], (b"-D",)),
                        (["-D", "3", "-e", "none"], (b"-e", b"-D")), (["-D", "3", "-e", "53"], (b"-e", b"-D"))):
        r = ma_hip(path, args)
        assert r.returncode == 1 and r.stdout == b"" and len(r.stderr.strip().split(b"\n")) == 1, (args, r.stderr)
        assert all(w in r.stderr for w in words), (args, r.stderr)
    assert ok(path, ["-S", "-f", "95"]).startswith(b"# ma_hip damage classes")                      # -S with -f 95 alone is fine
    for fmt in ("3", "94"):
        r = ma_hip(path, ["-f", fmt])
        assert r.returncode != 0 and b"outside the MI355X-accelerated path" in r.stderr and b"95" in r.stderr and r.stdout == b""


def test_d_is_still_parsed_and_ignored_and_the_help_names_the_new_options(tmp_path):
    path = write(dc.case("hand")[0], str(tmp_path / "in.maln"))
    assert ok(path, ["-d"]) == ok(path, ["-f", "1"]) and ok(path, ["-d", "-f", "41"]) == ok(path, ["-f", "41"])
    r = subprocess.run([MA], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0 and all(w in r.stdout for w in (b"-D", b"-e", b"-S", b"95"))


def test_the_run_without_the_new_options_is_unchanged(tmp_path):
    """-f 41 against the reference's recorded output (tests/golden/ma_synth), -u -f 41 against the reference's recorded output for the
    file the duplicate filter's restatement reduced (tests/golden/ma_dedup), -f 9 -- a report the reference does not have, so no
    recorded bytes exist -- against tests/ma_profile_ref.py, which the profile's own tests hold it to"""
    from test_ma_synth_cpu import case, recorded
    for name in ("edge256", "codes_anc"):
        m, _ = case(name)
        path = write(m, str(tmp_path / (name + ".maln")))
        assert ok(path, ["-f", "41", "-c", "1"]) == recorded(name, "f41c1")[0].encode("latin1"), name
        assert ok(path, ["-f", "9"]).decode() == ma_profile_ref.table(m), name
    with gzip.open(os.path.join(ROOT, "tests", "golden", "ma_dedup", "outputs.json.gz")) as f:
        dedup = json.load(f)["cases"]
    for name in ("hand", "wrap"):
        path = write(maln_dedup_cases.case(name), str(tmp_path / (name + ".maln")))
        assert ok(path, ["-u", "-f", "41", "-c", "1"]) == dedup[name]["0"]["f41c1"].encode("latin1"), name
