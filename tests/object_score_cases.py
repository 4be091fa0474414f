"""What the object-score tests share (tests/test_object_scores_host.py, tests/test_hip_object_scores.py): an oracle that uses neither
route of utilities/object_scores.py - a dict of key counts filled voxel by voxel, and the runs counted in the same loop, written
from the definitions - the root volumes the overlap table is checked on, hand-built scenes with known answers, and the vessels
pair of the committed digest.  Everything is built once and never written to."""
import functools
import hashlib
import json
import math
from pathlib import Path

import numpy as np

import components_cases as cc

GOLDEN = Path(__file__).resolve().parent / "golden"


# ---- the oracle ------------------------------------------------------------------------------------------------------------------
def oracle_table(a, b, skip=None):
    """((a, b, count) sorted by (a, b), runs) of two root volumes, voxel by voxel in plain Python"""
    a, b = np.asarray(a), np.asarray(b)
    row = a.shape[-1]
    fa, fb = a.reshape(-1).tolist(), b.reshape(-1).tolist()
    fs = [0] * len(fa) if skip is None else np.asarray(skip).reshape(-1).astype(np.int64).tolist()
    counts, runs, before = {}, 0, None
    for v, (ka, kb, s) in enumerate(zip(fa, fb, fs)):
        if v % row == 0:
            before = None                       # a row starts: no voxel before this one
        key = None if s else (ka << 32) | kb
        if key is not None:
            counts[key] = counts.get(key, 0) + 1
            runs += key != before
        before = key
    keys = sorted(counts)
    return (np.array([k >> 32 for k in keys], dtype=np.int64), np.array([k & 0xFFFFFFFF for k in keys], dtype=np.int64),
            np.array([counts[k] for k in keys], dtype=np.int64)), runs


def oracle_partition(a, b, count):
    """(H(P|T), H(T|P), adapted Rand error) of a table, from the definitions with exact sums"""
    from fractions import Fraction
    rows, cols = {}, {}
    for i, j, n in zip(a.tolist(), b.tolist(), count.tolist()):
        rows[i], cols[j] = rows.get(i, 0) + n, cols.get(j, 0) + n
    total = sum(rows.values())
    split = math.fsum(-(n / total) * math.log2(n / rows[i]) for i, j, n in zip(a.tolist(), b.tolist(), count.tolist()))
    merge = math.fsum(-(n / total) * math.log2(n / cols[j]) for i, j, n in zip(a.tolist(), b.tolist(), count.tolist()))
    both = sum(n * n for n in count.tolist())
    p, r = Fraction(both, sum(n * n for n in cols.values())), Fraction(both, sum(n * n for n in rows.values()))
    return split, merge, float(1 - 2 * p * r / (p + r))


def assert_tables_equal(got, want, what=""):
    for g, w, name in zip(got, want, ("a", "b", "count")):
        assert g.dtype == np.int64 and g.shape == w.shape and np.array_equal(g, w), (what, name)


def table_digest(table) -> str:
    return hashlib.sha256(b"".join(np.ascontiguousarray(x, dtype=np.int64).tobytes() for x in table)).hexdigest()


# ---- root volumes for the sweep ---------------------------------------------------------------------------------------------------
def _roots(labels, connectivity=6):
    return cc.oracle_roots(np.asarray(labels, dtype=np.uint8), connectivity)


def _coherent(shape, seed, k=3):
    """labels with runs a few voxels long along x, so that runs end at row ends and cross the 64-lane boundary"""
    rng = np.random.default_rng(seed)
    z, y, x = shape
    coarse = rng.integers(0, k, size=(z, y, (x + 6) // 7 + 1), dtype=np.uint8)
    return np.ascontiguousarray(np.repeat(coarse, 7, axis=2)[:, :, seed % 5:seed % 5 + x])


@functools.lru_cache(maxsize=None)
def sweep_volumes():
    """[(name, a, b, skip or None)]: int32 root volumes, read-only"""
    out = []
    seed = 0
    for x in (1, 63, 64, 65, 130):
        for z in (1, 2, 5):
            for y in (1, 2, 5):
                seed += 1
                la, lb = _coherent((z, y, x), seed), _coherent((z, y, x), 100 + seed)
                skip = None if seed % 3 else _coherent((z, y, x), 200 + seed, k=4) == 0
                out.append((f"{z}x{y}x{x}", _roots(la), _roots(lb), skip))
    rng = np.random.default_rng(11)
    # 4 x 33 x 257 = 33924 voxels: more than one workgroup's span of 32768 and no multiple of it, of 256 or of 64
    la, lb = _coherent((4, 33, 257), 7), _coherent((4, 33, 257), 8)
    out.append(("4x33x257 past one workgroup", _roots(la), _roots(lb), None))
    out.append(("4x33x257 past one workgroup, skips", _roots(la), _roots(lb), rng.random((4, 33, 257)) < 0.2))
    # thousands of distinct keys: the hash collides and probes; debris takes the per-run path
    ra, rb = rng.integers(0, 4, (17, 19, 67), dtype=np.uint8), rng.integers(0, 4, (17, 19, 67), dtype=np.uint8)
    out.append(("17x19x67 random K=4", _roots(ra), _roots(rb), None))
    out.append(("17x19x67 random K=4, 26-connected", _roots(ra, 26), _roots(rb, 26), None))
    # one key, one slot: the run-length adds carry everything
    solid = np.zeros((5, 33, 257), dtype=np.int32)
    out.append(("two solid volumes", solid, solid.copy(), None))
    # roots need not be small: the largest values a volume below 2^31 voxels can hold, in both halves of the key
    big = np.array([0, 1, (1 << 31) - 1, (1 << 31) - 2, 1 << 30], dtype=np.int32)
    out.append(("keys with high bits", big[rng.integers(0, 5, (3, 7, 70))], big[rng.integers(0, 5, (3, 7, 70))], None))
    # skip: whole rows, single voxels inside a run (it breaks and restarts), everything
    la = _coherent((3, 6, 130), 21)
    rows = np.zeros((3, 6, 130), dtype=bool)
    rows[:, 1::2] = True
    out.append(("skip whole rows", _roots(la), _roots(la), rows))
    single = np.zeros((3, 6, 130), dtype=bool)
    single[:, :, 3::9] = True
    single[:, :, 64] = True
    ones = np.zeros((3, 6, 130), dtype=np.int32)
    out.append(("skip single voxels inside a run", ones, ones.copy(), single))
    out.append(("skip single voxels, coherent labels", _roots(la), _roots(_coherent((3, 6, 130), 22)), single))
    out.append(("skip everything", _roots(la), _roots(la), np.ones((3, 6, 130), dtype=bool)))
    for _, a, b, skip in out:
        a.setflags(write=False)
        b.setflags(write=False)
        if skip is not None:
            skip.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def sweep_expected():
    """the oracle's (table, runs) per sweep volume, computed once"""
    return [oracle_table(a, b, skip) for _, a, b, skip in sweep_volumes()]


@functools.lru_cache(maxsize=None)
def hundred_keys():
    """(a, b): 1 x 4 x 112 roots with 112 distinct keys in runs of 4 - for the table that is too small"""
    a = (np.arange(448, dtype=np.int32) // 4).reshape(1, 4, 112)
    return a, np.ascontiguousarray(a[:, ::-1, :])


# ---- hand-built scenes ---------------------------------------------------------------------------------------------------------------
def _scene():
    return np.zeros((4, 6, 24), dtype=np.uint8)


def hand_cases():
    """[(name, pred, truth, keyword arguments of object_overlaps, expected figures of class 1 at IoU 0.5 as a dict)] - two classes,
    background not scored.  ``partition``: None, or the (vi_split, vi_merge, adapted_rand_error) known by hand"""
    cases = []
    bar = _scene()
    bar[1, 2, 2:12] = 1                                   # one true object of 10 voxels
    # cut in two, 7 + 2: the larger piece has IoU 7 / 10 and matches
    p = bar.copy()
    p[1, 2, 9] = 0
    cases.append(("split, larger piece matches", p, bar, {}, dict(true=1, pred=2, tp=1, fp=1, fn=0, splits=1, merges=0, ious=[0.7]), None))
    # cut in two, 5 + 4: the larger piece has IoU 5 / 10 = 1 / 2 exactly - not above 0.5, no match
    p = bar.copy()
    p[1, 2, 7] = 0
    cases.append(("split, iou exactly one half", p, bar, {}, dict(true=1, pred=2, tp=0, fp=2, fn=1, splits=1, merges=0, ious=[]), None))
    # two true objects bridged by the prediction
    t = _scene()
    t[1, 2, 2:8] = 1
    t[1, 2, 10:16] = 1
    p = t.copy()
    p[1, 2, 8:10] = 1
    cases.append(("two objects bridged", p, t, {}, dict(true=2, pred=1, tp=0, fp=1, fn=2, splits=0, merges=1, ious=[]), None))
    # an invented object
    p = bar.copy()
    p[3, 4, 15:20] = 1
    cases.append(("an invented object", p, bar, {}, dict(true=1, pred=2, tp=1, fp=1, fn=0, splits=0, merges=0, ious=[1.0]), None))
    # a missed one
    t = bar.copy()
    t[3, 4, 15:20] = 1
    cases.append(("a missed object", bar, t, {}, dict(true=2, pred=1, tp=1, fp=0, fn=1, splits=0, merges=0, ious=[1.0]), None))
    # a predicted object wholly inside the ignore label, and the ignored region itself: gone from both sides
    t = bar.copy()
    t[3, 3:6, 14:22] = 9
    p = bar.copy()
    p[3, 4, 15:20] = 1
    cases.append(("an object inside the ignore label", p, t, dict(label_values=[0, 1], ignore_label=9),
                  dict(true=1, pred=1, tp=1, fp=0, fn=0, splits=0, merges=0, ious=[1.0]), (0.0, 0.0, 0.0)))
    # identical volumes
    t = bar.copy()
    t[3, 4, 15:20] = 1
    cases.append(("identical volumes", t, t.copy(), {}, dict(true=2, pred=2, tp=2, fp=0, fn=0, splits=0, merges=0, ious=[1.0, 1.0]), (0.0, 0.0, 0.0)))
    # half of a 4-voxel object: IoU 2 / 4
    t = _scene()
    t[2, 2, 4:8] = 1
    p = _scene()
    p[2, 2, 4:6] = 1
    cases.append(("half an object, iou exactly one half", p, t, {}, dict(true=1, pred=1, tp=0, fp=1, fn=1, splits=0, merges=0, ious=[]), None))
    return cases


def check_hand_case(scores, expected, partition):
    c = scores["classes"][1]
    row = c["thresholds"][0]
    got = dict(true=c["true_objects"], pred=c["predicted_objects"], tp=row["tp"], fp=row["fp"], fn=row["fn"], splits=c["splits"], merges=c["merges"])
    assert got == {k: expected[k] for k in got}, got
    tp, fp, fn, ious = expected["tp"], expected["fp"], expected["fn"], expected["ious"]
    want = dict(precision=tp / (tp + fp) if tp + fp else math.nan, recall=tp / (tp + fn) if tp + fn else math.nan,
                f1=2 * tp / (2 * tp + fp + fn), sq=math.fsum(ious) / tp if tp else math.nan, pq=math.fsum(ious) / (tp + fp / 2 + fn / 2))
    for name, value in want.items():
        assert (math.isnan(row[name]) and math.isnan(value)) or abs(row[name] - value) <= 1e-15, (name, row[name], value)
    assert scores["classes"][0]["true_objects"] == 0 and math.isnan(scores["classes"][0]["thresholds"][0]["f1"])       # background is not scored
    if partition is not None:
        p = scores["partition"]
        assert (p["vi_split"], p["vi_merge"], p["adapted_rand_error"]) == partition


# ---- the vessels pair ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def vessels_pair():
    """(pred, truth), uint8 class indices: truth is the committed vessels labels (> 0); the prediction is the truth shifted by one
    voxel along x, with plane y = 128, plane z = 96 and the corner [:64, :64, :64] cleared"""
    truth = (cc.vessels() > 0).astype(np.uint8)
    pred = np.zeros_like(truth)
    pred[:, :, 1:] = truth[:, :, :-1]
    pred[:, 128, :] = 0
    pred[96] = 0
    pred[:64, :64, :64] = 0
    truth.setflags(write=False)
    pred.setflags(write=False)
    return pred, truth


@functools.lru_cache(maxsize=None)
def vessels_expected():
    return json.loads((GOLDEN / "object_scores_vessels.json").read_text())


def rows_with_one_background(overlaps) -> int:
    """the table's rows when all background components of a side count as ONE segment - what labelling the foreground alone
    (scipy.ndimage.label of ``> 0``) gives, and the figure the vessels check was first made with"""
    t_class = dict(zip(overlaps["truth_roots"].tolist(), overlaps["truth_classes"].tolist()))
    p_class = dict(zip(overlaps["pred_roots"].tolist(), overlaps["pred_classes"].tolist()))
    return len({(a if t_class[a] else -1, b if p_class[b] else -1) for a, b in zip(overlaps["a"].tolist(), overlaps["b"].tolist())})


def vessels_digest(overlaps, scores) -> dict:
    """what the committed digest holds of one run: integers, the table's hash, and the float figures"""
    c = scores["classes"][1]
    row = c["thresholds"][0]
    return dict(true_objects=c["true_objects"], predicted_objects=c["predicted_objects"], table_rows=scores["table_rows"],
                table_rows_one_background=rows_with_one_background(overlaps), tp=row["tp"], fp=row["fp"], fn=row["fn"], splits=c["splits"],
                merges=c["merges"], runs=scores["runs"], table_sha256=table_digest((overlaps["a"], overlaps["b"], overlaps["count"])),
                f1=row["f1"], sq=row["sq"], pq=row["pq"], vi_split=scores["partition"]["vi_split"], vi_merge=scores["partition"]["vi_merge"],
                adapted_rand_error=scores["partition"]["adapted_rand_error"])


VESSELS_RUNS = {"connectivity_6": dict(connectivity=6, swapped=False), "connectivity_6_swapped": dict(connectivity=6, swapped=True),
                "connectivity_26": dict(connectivity=26, swapped=False)}
