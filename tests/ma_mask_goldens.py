"""What tools/make_ma_mask_goldens.py and the tests share about tests/golden/ma_mask: the committed, reference-written inputs, and the
rare paths the fixtures must show together, judged by the restatement (tests/ma_mask_ref.py) alone."""
import gzip
import os

import ma_mask_ref as ref
import maln_synth as ms

INPUTS = {"fix_c_anc": ("maln", "fix_c_anc.1"), "indel_anc_k12": ("maln", "indel_anc_k12.1"), "d150_anc_k12": ("maln", "d150_anc_k12.1"),
          "s150_full": ("maln", "s150_full.1"), "reads_a": ("ma_damage", "reads_a.maln.1.gz")}
RUNS = (("f41c1", ["-f", "41", "-c", "1"]), ("f5", ["-f", "5"]), ("f1", ["-f", "1"]))
_loaded = {}


def text(name):
    """the file as `ma` reads it, first line included"""
    folder, fn = INPUTS[name]
    path = os.path.join(ms.GOLDEN, folder, fn)
    if fn.endswith(".gz"):
        with gzip.open(path, "rb") as f:
            return f.read().decode("latin1")
    with open(path, encoding="latin1") as f:
        return ms.MA_HEADER + f.read()


def load(name):
    if name not in _loaded:
        _loaded[name] = ms.parse_maln(text(name).split("\n", 1)[1])
    return _loaded[name]


def e_args(n5, n3, substitute, ss):
    return ["-E", "%d,%d" % (n5, n3)] + (["-x"] if substitute else []) + (["-S"] if ss else [])


def rare_paths(masks):
    """masks: {file: {tag: (Maln, Masked)}}.  The list of what the set fails to show (empty: it is a fixture)"""
    emptied = dropped = moved = stripped = 0
    ends = set()
    halves = set()
    for name, by_tag in masks.items():
        for tag, (m, got) in by_tag.items():
            emptied += sum(got.emptied)
            dropped += got.pairs_dropped
            stripped += got.stripped
            for strand in (0, 1):
                for end in (0, 1):
                    if got.hist[strand, end].sum():
                        ends.add((strand, end))
            old = [p for r in m.rec for p, _ in r["ins"]]
            moved += sum(1 for k, p in zip(got.pair_keep.tolist(), zip(old, got.ins_pos.tolist())) if k and p[0] != p[1])
            halves |= {r["seg"] for r, c in zip(m.rec, got.count.tolist()) if c and r["seg"] in "fb" and c < r["end"] - r["start"] + 1}
    missing = []
    if emptied < 2:
        missing.append("two emptied records")
    if dropped < 5:
        missing.append("five dropped pairs")
    if moved < 5:
        missing.append("five pairs kept with a changed position")
    if stripped < 1:
        missing.append("a stripped '-' column")
    if len(ends) < 4:
        missing.append("forward and RC records with counts at both ends")
    if halves != {"f", "b"}:
        missing.append("trimmed f and b halves")
    return missing


def all_masks():
    return {name: {ref.tag(*s): (load(name), ref.mask(load(name), *s)) for s in ref.SETTINGS} for name in INPUTS}
