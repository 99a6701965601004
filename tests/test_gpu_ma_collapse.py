"""The duplicate consensus on the GPU: MiaHip.ma_collapse (mia_hip_ma_collapse: plan, count, decide -- csrc/mia_ma_collapse_kernels.h)
must give exactly SEQ', members, the counts and the totals of tests/ma_collapse_ref.py, the rule of DESIGN.md ("Duplicate consensus")
restated as plain loops, for every shape of tests/maln_collapse_cases.py and every tolerance; and ma_hip -u -j [-t N] must print, byte
for byte, what the compiled reference's ma printed for the file the restatement collapsed (tests/golden/ma_collapse)."""
import ctypes as C
import gzip
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import ma_collapse_ref as ref
import ma_dedup_ref as ddref
import maln_collapse_cases as cc
import maln_synth as ms
from conftest import ROOT

pytestmark = pytest.mark.gpu

MA = os.path.join(ROOT, "mapping-iterative-assembler_amd", "ma_hip")
GOLD = os.path.join(ROOT, "tests", "golden", "ma_collapse")
ERR_ARG, ERR_STATE = -2, -4                # MIA_HIP_ERR_ARG, MIA_HIP_ERR_STATE (include/mia_hip.h)
FORMATS = (("f41c1", ["-f", "41", "-c", "1"]), ("f5", ["-f", "5"]), ("f1", ["-f", "1"]))
_want, _gold = {}, []


def want(name, t, voting=True):
    """the restatement's (records, keep, members, hist, n_collapsed, n_changed, totals), once per case and tolerance"""
    if (name, t, voting) not in _want:
        m = cc.case(name)
        _want[name, t, voting] = ref.collapse_records(m, t, ref.not_dropped(m) if voting else None)
    return _want[name, t, voting]


def gold():
    if not _gold:
        with gzip.open(os.path.join(GOLD, "outputs.json.gz")) as f:
            _gold.append(json.load(f))
    return _gold[0]


@pytest.fixture(scope="module")
def hip():
    import mia_amd
    return mia_amd.MiaHip(0)


def tally(hip, m):
    hip.set_pssm(m.fpsm, m.rpsm)
    hip.ma_tally(*ms.ma_tally_args(ms.flatten(m)))


def seq_of(recs):
    return np.frombuffer("".join(r["seq"][:r["end"] - r["start"] + 1] for r in recs).encode("latin1"), np.uint8)


def check(got, wanted, what):
    seq, members, hist, n_collapsed, n_changed = got
    assert (n_collapsed, n_changed) == (wanted[4], wanted[5]), what
    assert np.array_equal(hist, wanted[3]), (what, hist.tolist(), wanted[3].tolist())
    bad = np.nonzero(members != wanted[2])[0]
    assert bad.size == 0, (what, "members", bad[:5].tolist())
    exp = seq_of(wanted[0])
    assert len(seq) == len(exp), what
    bad = np.nonzero(seq != exp)[0]
    assert bad.size == 0, (what, "SEQ'", bad[:5].tolist(), bytes(seq[bad[:5]]), bytes(exp[bad[:5]]))


@pytest.mark.parametrize("name", cc.CASES + cc.LIBRARY_ONLY)
def test_library_call_matches_the_restatement(hip, name):
    m = cc.case(name)
    tally(hip, m)
    arrays = ddref.device_arrays(m.rec)
    for t in (0,) if name in cc.LIBRARY_ONLY else cc.TOLERANCES:
        hip.ma_dedup(m.L, *arrays, t)
        check(hip.ma_collapse(None, ref.not_dropped(m)), want(name, t), "%s t=%d" % (name, t))
    seq = hip.ma_collapse(None, ref.not_dropped(m))[0]
    changed = int((seq != seq_of(m.rec)).sum())
    assert changed == want(name, cc.TOLERANCES[-1] if name not in cc.LIBRARY_ONLY else 0)[5], name       # n_changed is the bytes that differ


@pytest.mark.parametrize("name", ("hand", "votes", "dropped", "sizes"))
def test_no_vote_array_is_everyone_votes(hip, name):
    m = cc.case(name)
    tally(hip, m)
    hip.ma_dedup(m.L, *ddref.device_arrays(m.rec), 0)
    a = hip.ma_collapse(None, None)
    b = hip.ma_collapse(None, np.ones(len(m.rec), np.uint8))
    for x, y in zip(a, b):
        assert np.array_equal(x, y), name
    check(a, want(name, 0, voting=False), name + " everyone votes")
    if name != "sizes":                                              # (these cases hold dropped records)
        assert not np.array_equal(a[0], hip.ma_collapse(None, ref.not_dropped(m))[0]), name


@pytest.mark.parametrize("name,t", (("sizes", 1), ("wrap", 7), ("jitter", 2), ("mixed", 0)))
def test_a_shuffled_file_through_rec_of(hip, name, t):
    """the tallied records are the file's records sorted by START and END, as ma_hip hands them over; the filter gets the file's own
    order, which decides ties, and rec_of says where each of its records went"""
    m = cc.case(name)
    order = sorted(range(len(m.rec)), key=lambda i: (m.rec[i]["start"], m.rec[i]["end"]))            # (stable)
    twin = ms.Maln()
    twin.__dict__.update(m.__dict__)
    twin.rec = [m.rec[i] for i in order]
    rec_of = np.empty(len(order), np.int64)
    rec_of[order] = np.arange(len(order))
    tally(hip, twin)
    hip.ma_dedup(m.L, *ddref.device_arrays(m.rec), t)
    seq, members, hist, n_collapsed, n_changed = hip.ma_collapse(rec_of, ref.not_dropped(twin))
    w = want(name, t)
    assert (n_collapsed, n_changed) == (w[4], w[5]) and np.array_equal(hist, w[3])
    assert np.array_equal(members, w[2][order])
    assert np.array_equal(seq, seq_of([w[0][i] for i in order]))


def test_twice_on_one_context(hip):
    """buffers are reused: large, small, nothing to launch, large again"""
    for name, t in (("mixed", 2), ("hand", 0), ("one", 0), ("pile_5000", 1), ("empty", 0), ("mixed", 0)):
        m = cc.case(name)
        tally(hip, m)
        hip.ma_dedup(m.L, *ddref.device_arrays(m.rec), t)
        check(hip.ma_collapse(None, ref.not_dropped(m)), want(name, t), "%s t=%d in a row" % (name, t))


def test_without_a_cluster_of_two_nothing_is_launched(hip):
    for name in ("singletons", "one", "empty"):
        m = cc.case(name)
        tally(hip, m)
        hip.ma_dedup(m.L, *ddref.device_arrays(m.rec), 0)
        hip.stage_stats(reset=True)
        seq, members, hist, n_collapsed, n_changed = hip.ma_collapse()
        assert np.array_equal(seq, seq_of(m.rec)) and not members.any() and not hist.any() and (n_collapsed, n_changed) == (0, 0)
        st = hip.stage_stats()
        assert all(st[k][1] == 0 for k in hip.STAGES_ALWAYS_TIMED), name
    m = cc.case("hand")
    tally(hip, m)
    hip.ma_dedup(m.L, *ddref.device_arrays(m.rec), 0)
    hip.stage_stats(reset=True)
    hip.ma_collapse()
    st = hip.stage_stats()
    assert st["k_ma_collapse_plan"][1] == 2 and st["k_ma_collapse_count"][1] == 1        # every stage goes through the stage timers
    assert list(st)[:len(hip.STAGES)] == hip.STAGES and list(st)[len(hip.STAGES):] == hip.STAGES_ALWAYS_TIMED


def test_argument_and_state_errors():
    import mia_amd
    hip = mia_amd.MiaHip(0)
    lib, h = hip._l, hip._h
    n1, n2 = C.c_int64(), C.c_int64()

    def call(rec_of=None):
        p = None if rec_of is None else np.ascontiguousarray(rec_of, np.int64).ctypes.data_as(C.c_void_p)
        return lib.mia_hip_ma_collapse(h, p, None, C.byref(n1), C.byref(n2))

    def getter():
        return lib.mia_hip_get_ma_collapse(h, None, 0, None, None)

    m, other = cc.case("hand"), cc.case("votes")
    arrays = ddref.device_arrays(m.rec)
    assert call() == ERR_STATE and getter() == ERR_STATE                         # neither a tally nor a filter
    hip.ma_dedup(m.L, *arrays, 0)
    assert call() == ERR_STATE and b"ma_tally" in lib.mia_hip_last_error(h)      # no tally
    tally(hip, m)
    assert call() == ERR_STATE and b"older" in lib.mia_hip_last_error(h)         # the filter is older than the tally
    hip.ma_dedup(other.L, *ddref.device_arrays(other.rec), 0)
    assert call() == ERR_ARG and b"numbers of records" in lib.mia_hip_last_error(h)
    hip.ma_dedup(m.L, *arrays, 0)
    n = len(m.rec)
    for bad in (np.zeros(n), np.r_[np.arange(n - 1), n], np.r_[np.arange(n - 1), -1], np.r_[0, np.arange(n - 1)]):
        assert call(bad) == ERR_ARG and b"permutation" in lib.mia_hip_last_error(h)
        assert getter() == ERR_STATE                                             # a refused call leaves no result
    swapped = np.arange(n)
    swapped[[0, 3]] = [3, 0]                                                     # a permutation, but records 0 and 3 have other coordinates
    assert call(swapped) == ERR_ARG and b"disagrees" in lib.mia_hip_last_error(h)
    start, end = arrays[0].copy(), arrays[1].copy()
    end[0] -= 1
    hip.ma_dedup(m.L, start, end, *arrays[2:], 0)
    assert call() == ERR_ARG and b"disagrees" in lib.mia_hip_last_error(h)       # END is not start + columns - 1
    hip.ma_dedup(m.L, *arrays, 0)
    assert call() == 0 and getter() == 0                                         # every pointer may be NULL
    assert lib.mia_hip_ma_collapse(h, None, None, None, None) == 0
    seq = np.zeros(4, np.uint8)
    assert lib.mia_hip_get_ma_collapse(h, seq.ctypes.data_as(C.c_void_p), 4, None, None) == ERR_ARG      # too small a buffer
    check(hip.ma_collapse(None, ref.not_dropped(m)), want("hand", 0), "hand after the refusals")
    hip.ma_dedup(m.L, *arrays, 0)
    assert getter() == ERR_STATE                                                 # the next filter invalidates the result
    assert call() == 0
    tally(hip, m)
    assert getter() == ERR_STATE and call() == ERR_STATE                         # ... and so does the next tally


# ---- ma_hip ------------------------------------------------------------------------------------------------------------------------
def write(m, path):
    with open(path, "w", encoding="latin1") as f:
        f.write(ms.MA_HEADER + ms.write_maln(m))
    return path


def ma_hip(path, args):
    return subprocess.run([MA, "-M", path] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


def same_as_recorded(out, recorded, what):
    if isinstance(recorded, dict):
        assert (len(out), hashlib.sha256(out).hexdigest()) == (recorded["bytes"], recorded["sha256"]), what
    else:
        assert out == recorded.encode("latin1"), what


def table_of(hist, totals, t):
    n_mol, n_clu, orphans = totals
    hist = np.asarray(hist).reshape(2, 6, 6)
    out = ["# ma_hip duplicate consensus: %d molecules, %d clusters, %d collapsed, %d orphans, tolerance %d\n" % (n_mol, n_clu, int(hist[:, :, 0].sum()), orphans, t),
           "# size\tstrand\tclusters\tcolumns\tsplit\tto_base\tto_gap\tto_N\n"]
    for b, label in enumerate(ref.SIZE_BINS):
        for strand in (0, 1):
            out.append("%s\t%s\t%s\n" % (label, "-" if strand else "+", "\t".join(str(int(x)) for x in hist[strand, b])))
    return "".join(out).encode()


@pytest.mark.parametrize("t", (0, 2))
@pytest.mark.parametrize("name", cc.CASES)
def test_ma_hip_u_j_prints_what_the_reference_printed_for_the_collapsed_file(name, t, tmp_path):
    m = cc.case(name)
    path = write(m, str(tmp_path / "in.maln"))
    extra = ["-u", "-j"] + (["-t", str(t)] if t else [])
    recorded = gold()["cases"][name][str(t)]
    for tag, args in FORMATS:
        r = ma_hip(path, args + extra)
        assert r.returncode == 0, (args, r.stderr[-300:])
        same_as_recorded(r.stdout, recorded[tag], (name, t, tag))
    w = want(name, t)
    assert np.array_equal(np.array(recorded["hist"]).reshape(2, 6, 6), w[3])
    out = str(tmp_path / "out.maln")
    r = ma_hip(path, extra + ["-f", "98", "-m", out])
    assert r.returncode == 0, r.stderr[-300:]
    assert r.stdout == ref.report(m, t, ref.not_dropped(m)).encode() == table_of(w[3], w[6], t), (name, t)
    # -m: the restatement's file, its records in the order read_ma sorts them into, a missing NUM_INPUTS line read as 1
    new = ref.collapse(m, t, ref.not_dropped(m))[0]
    new.rec = [dict(r, num_inputs=1 if r["num_inputs"] is None else r["num_inputs"]) for r in sorted(new.rec, key=lambda r: (r["start"], r["end"]))]
    assert open(out, encoding="latin1").read().split("\n", 1)[1] == ms.write_maln(new), (name, t, "-m")


@pytest.mark.parametrize("t", (0, 2))
@pytest.mark.parametrize("name", ("reads_a", "reads_b"))
def test_ma_hip_u_j_on_the_references_own_runs(name, t, tmp_path):
    """tests/golden/ma_dedup/<set>.maln.1.gz is the compiled reference's `mia -c -n -H 1` on a read set; outputs.json.gz, "sets", holds
    its `ma` on the file the restatement collapsed"""
    path = str(tmp_path / "in.maln")
    with gzip.open(os.path.join(ROOT, "tests", "golden", "ma_dedup", name + ".maln.1.gz"), "rb") as f, open(path, "wb") as g:
        g.write(f.read())
    recorded = gold()["sets"][name][str(t)]
    extra = ["-u", "-j"] + (["-t", str(t)] if t else [])
    for tag, args in FORMATS:
        r = ma_hip(path, args + extra)
        assert r.returncode == 0, (args, r.stderr[-300:])
        same_as_recorded(r.stdout, recorded[tag], (name, t, tag))
    r = ma_hip(path, extra + ["-f", "98"])
    m = ms.parse_maln(open(path, encoding="latin1").read().split("\n", 1)[1])
    assert r.returncode == 0 and r.stdout == ref.report(m, t, ref.not_dropped(m)).encode(), (name, t)
    assert np.array_equal(np.array(recorded["hist"]).reshape(2, 6, 6), ref.collapse_records(m, t, ref.not_dropped(m))[3])


def test_a_minority_c_to_t_in_the_kept_copy_no_longer_makes_the_cluster_deaminated(tmp_path):
    m = cc.case("minority_ct")
    path = write(m, str(tmp_path / "in.maln"))
    outs = {}
    for tag, extra in (("u", ["-u"]), ("uj", ["-u", "-j"])):
        out = str(tmp_path / (tag + ".maln"))
        r = ma_hip(path, extra + ["-D", "3", "-f", "5", "-m", out])
        assert r.returncode == 0, r.stderr[-300:]
        outs[tag] = open(out, encoding="latin1").read().split("\n", 1)[1]
    assert outs["u"].startswith("MALN_NAS 1\n") and outs["uj"].startswith("MALN_NAS 0\n")
    r = ma_hip(path, ["-u", "-j", "-f", "5", "-m", str(tmp_path / "j.maln")])
    got = ms.parse_maln(open(str(tmp_path / "j.maln"), encoding="latin1").read().split("\n", 1)[1])
    assert [(x["id"], x["seq"][0], x["num_inputs"]) for x in got.rec] == [("kept", "C", 3)]


def test_j_needs_u_and_f98_needs_j(tmp_path):
    path = write(cc.case("hand"), str(tmp_path / "in.maln"))
    r = ma_hip(path, ["-j", "-f", "41"])
    assert r.returncode == 1 and b"-j" in r.stderr and b"-u" in r.stderr and r.stdout == b"" and r.stderr.count(b"\n") == 1
    r = ma_hip(path, ["-u", "-f", "98"])
    assert r.returncode == 1 and b"-f 98" in r.stderr and b"-j" in r.stderr and r.stdout == b"" and r.stderr.count(b"\n") == 1
    r = ma_hip(path, ["-f", "99"])
    assert r.returncode == 1 and b"outside the MI355X-accelerated path" in r.stderr and b"98" in r.stderr
    r = subprocess.run([MA], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert b"-j" in r.stdout and b"98" in r.stdout
    empty = write(cc.case("empty"), str(tmp_path / "empty.maln"))
    r = ma_hip(empty, ["-u", "-j", "-f", "98"])
    assert r.returncode == 0 and r.stdout == ref.report(cc.case("empty"), 0).encode() and r.stdout.count(b"\n") == 14


def test_without_j_the_outputs_of_u_are_the_recorded_ones(tmp_path):
    path = str(tmp_path / "in.maln")
    with gzip.open(os.path.join(ROOT, "tests", "golden", "ma_dedup", "reads_a.maln.1.gz"), "rb") as f, open(path, "wb") as g:
        g.write(f.read())
    with gzip.open(os.path.join(ROOT, "tests", "golden", "ma_dedup", "outputs.json.gz")) as f:
        sets = json.load(f)["sets"]["reads_a"]
    for tag, args in (("f41c1", ["-f", "41", "-c", "1"]), ("f5c1", ["-f", "5", "-c", "1"]), ("f5c2", ["-f", "5", "-c", "2"])):
        r = ma_hip(path, ["-u"] + args)
        assert r.returncode == 0 and r.stdout == sets[tag].encode("latin1"), tag
