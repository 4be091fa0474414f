"""Object-level scores of a predicted label volume against a labelled one: how many of the true objects were found, split, merged or
invented - detection precision / recall / F1 at an IoU threshold, panoptic quality, split and merge counts, variation of
information and the adapted Rand error.

Definitions.  Volumes, connectivity, components and roots are those of ``utilities/components.py``; truth values map to classes as
in ``utilities/surface_distance.py`` (255 = ignore, 254 = no class) and predictions hold class indices.  Both volumes are labelled,
every value at once; a voxel whose truth is ignored is left out of everything below.  The OVERLAP TABLE is the list of (true
component, predicted component, voxels in both), sorted by the pair; a component's size is its row sum (truth) or column sum
(prediction), its class the class byte at its root.  The OBJECTS of class ``c`` are the components of class ``c`` with at least
``min_voxels`` voxels; class 0 has objects only with ``background``.  A true and a predicted object of the same class MATCH at the
threshold ``t`` when ``n / (|T| + |P| - n) > t``; for ``t >= 0.5`` an object has at most one match.  TP = matches, FP = predicted
objects without one, FN = true objects without one; precision = TP / (TP + FP), recall = TP / (TP + FN), F1 = 2 TP / (2 TP + FP +
FN), SQ = the mean IoU of the matches, PQ = sum IoU / (TP + FP / 2 + FN / 2).  A true object is SPLIT when it shares at least
``min_overlap`` voxels with two or more predicted objects of its class; a predicted object that does so with two or more true
objects is a MERGE.  Over the whole table, components of every class as the segments of two partitions of the voxels that are not
ignored: the variation of information ``H(P|T)`` (split) + ``H(T|P)`` (merge) in bits, and the adapted Rand error ``1 - 2 p r / (p +
r)`` with ``p = sum n_ij^2 / sum b_j^2`` and ``r = sum n_ij^2 / sum a_i^2``.

All routes give the same integers: ``vs_overlap_runs`` and ``vs_overlap_table`` (csrc/overlap.hip) on the roots of
``vs_label_components`` on a GPU, ``np.unique`` over the 64-bit keys on a host.  Every figure is computed in float64 (the Rand sums
in Python integers) from those integers alone, by the same code."""
from __future__ import annotations

import csv
import json
import math
from pathlib import Path

import numpy as np

from . import components as co
from . import evaluation as ev
from . import label_volume as lv

MIN_SLOTS = 64
_LOW = (1 << 32) - 1


# ---- the overlap table -------------------------------------------------------------------------------------------------------------
def split_keys(keys: np.ndarray, counts: np.ndarray):
    """sorted uint64 keys and their counts as the (a, b, count) int64 arrays of a table"""
    keys = np.asarray(keys, dtype=np.uint64)
    return (keys >> np.uint64(32)).astype(np.int64), (keys & np.uint64(_LOW)).astype(np.int64), np.asarray(counts, dtype=np.int64)


def _flat_int32(x, what: str):
    if tuple(x.shape) == () or int(np.prod(tuple(x.shape))) == 0:
        raise ValueError(f"{what}: expected a non-empty root volume")
    if lv.is_tensor(x):
        import torch
        if x.dtype != torch.int32:
            raise TypeError(f"{what}: roots are int32, got {x.dtype}")
        return x.contiguous().reshape(-1)
    x = np.asarray(x)
    if x.dtype != np.int32:
        raise TypeError(f"{what}: roots are int32, got {x.dtype}")
    return np.ascontiguousarray(x).reshape(-1)


def count_runs_host(a, b, skip, row: int) -> int:
    """the key runs along x, as ``vs_overlap_runs`` counts them"""
    a, b = np.asarray(a).reshape(-1, row), np.asarray(b).reshape(-1, row)
    live = np.ones(a.shape, dtype=bool) if skip is None else np.asarray(skip).reshape(-1, row) == 0
    start = live.copy()
    start[:, 1:] &= ~live[:, :-1] | (a[:, 1:] != a[:, :-1]) | (b[:, 1:] != b[:, :-1])
    return int(start.sum())


def table_host(a, b, skip):
    """the host route on flat arrays: ``np.unique`` over one 64-bit key per voxel that is not skipped"""
    keys = (a.astype(np.uint64) << np.uint64(32)) | b.astype(np.uint64)
    if skip is not None:
        keys = keys[skip == 0]
    return split_keys(*np.unique(keys, return_counts=True))


def device_inputs(a, b, skip, device):
    """flat root arrays or tensors, and the skip mask as uint8 or None, as aligned device memory"""
    import torch

    def dev(x):
        x = (x if lv.is_tensor(x) else torch.from_numpy(np.require(x, requirements="CW"))).to(device).contiguous()    # a read-only array is copied
        return x if x.data_ptr() % 16 == 0 else x.clone()

    if skip is not None:
        skip = dev(skip)
        if skip.dtype != torch.uint8:
            skip = (skip != 0).to(torch.uint8)
    return dev(a), dev(b), skip


def runs_device(a, b, skip, row: int) -> int:
    """vs_overlap_runs on flat device tensors"""
    import torch
    from .. import _lib
    runs = torch.empty(1, dtype=torch.int64, device=a.device)
    with torch.cuda.device(a.device):
        _lib.check(_lib.lib.vs_overlap_runs(_lib.ptr(a), _lib.ptr(b), _lib.ptr(skip), a.numel(), int(row), _lib.ptr(runs), _lib.stream_ptr()))
    return int(runs.item())


def table_slots(runs: int) -> int:
    """the power of two at or above twice the runs, at least 64: the table is at most half full"""
    return max(MIN_SLOTS, 1 << max(2 * int(runs) - 1, 0).bit_length())


def hash_device(a, b, skip, row: int, slots: int):
    """vs_overlap_table on flat device tensors: (keys, counts, used) as it left them, on the device"""
    import torch
    from .. import _lib
    keys = torch.empty(int(slots), dtype=torch.int64, device=a.device)
    counts = torch.empty(int(slots), dtype=torch.int64, device=a.device)
    used = torch.empty(2, dtype=torch.int64, device=a.device)
    with torch.cuda.device(a.device):
        _lib.check(_lib.lib.vs_overlap_table(_lib.ptr(a), _lib.ptr(b), _lib.ptr(skip), a.numel(), int(row), _lib.ptr(keys), _lib.ptr(counts),
                                             int(slots), _lib.ptr(used), _lib.stream_ptr()))
    return keys, counts, used


def table_device_sorted(a, b, skip, row: int):
    """the device route on flat device tensors, up to the table on the device: (int64 keys ascending, int64 counts).  The runs size
    the table, the kernel fills it, torch compacts and sorts the occupied slots"""
    import torch
    runs = runs_device(a, b, skip, row)
    slots = table_slots(runs)
    lv.require_memory(a.device, 16 * slots + 32 * min(runs, a.numel()), f"the overlap table of {runs} runs")
    keys, counts, used = hash_device(a, b, skip, row, slots)
    occupied = torch.nonzero(keys != -1).reshape(-1)                  # the free mark is all ones; a key's top bit is never set
    if int(occupied.numel()) != int(used[0]):
        raise RuntimeError(f"the overlap kernel claimed {int(used[0])} slots, the table holds {int(occupied.numel())} keys")
    keys, order = torch.sort(keys[occupied])
    return keys, counts[occupied][order]


def table_device(a, b, skip, row: int):
    """``table_device_sorted`` and the copy to the host: (a, b, count)"""
    keys, counts = table_device_sorted(a, b, skip, row)
    return split_keys(keys.cpu().numpy().view(np.uint64), counts.cpu().numpy())


def overlap_table_unique(a_roots, b_roots, skip=None, device=None):
    """The same table by ``torch.unique`` over one 64-bit key per voxel - a full sort of the volume: the device route there was before
    the kernel, kept as the baseline ``tools/overlap_probe.py`` measures against."""
    import torch
    device = lv.pick_device(device, a_roots, b_roots)
    if device is None:
        raise ValueError("overlap_table_unique is a device route: there is no GPU")
    a, b, skip = device_inputs(_flat_int32(a_roots, "a_roots"), _flat_int32(b_roots, "b_roots"), None if skip is None else skip.reshape(-1), device)
    keys = (a.to(torch.int64) << 32) | b.to(torch.int64)
    if skip is not None:
        keys = keys[skip == 0]
    keys, counts = torch.unique(keys, return_counts=True)
    return split_keys(keys.cpu().numpy().view(np.uint64), counts.cpu().numpy())


def overlap_table(a_roots, b_roots, skip=None, device=None):
    """(a, b, count), int64 arrays sorted by (a, b): for every pair of a root of ``a_roots`` and a root of ``b_roots`` (int32 root
    volumes of the same shape, host arrays or device tensors) that share a voxel, the number of voxels they share.  ``skip`` (same
    shape, bool or uint8, optional): a non-zero entry leaves the voxel out."""
    if tuple(a_roots.shape) != tuple(b_roots.shape) or (skip is not None and tuple(skip.shape) != tuple(a_roots.shape)):
        raise ValueError(f"root volumes of shapes {tuple(a_roots.shape)} and {tuple(b_roots.shape)}"
                         + ("" if skip is None else f" and a skip mask of shape {tuple(skip.shape)}") + ": the shapes must be equal")
    row = int(a_roots.shape[-1])
    device = lv.pick_device(device, a_roots, b_roots)
    a, b = _flat_int32(a_roots, "a_roots"), _flat_int32(b_roots, "b_roots")
    if a.shape[0] >= co.VOXEL_LIMIT:
        raise ValueError(f"{a.shape[0]} voxels: the overlap table needs fewer than 2^31")
    flat_skip = None if skip is None else skip.reshape(-1)
    if device is None:
        return table_host(lv.to_host(a), lv.to_host(b), None if flat_skip is None else lv.to_host(flat_skip))
    return table_device(*device_inputs(a, b, flat_skip, device), row)


# ---- the two labellings of a prediction and its ground truth -------------------------------------------------------------------------
def _class_list(classes):
    class_list = list(range(int(classes))) if np.isscalar(classes) else [int(c) for c in classes]
    if not class_list or min(class_list) < 0 or max(class_list) > 253:
        raise ValueError(f"classes must be 0..253, got {class_list[:20]}")
    return class_list


def object_overlaps(pred, truth, classes, *, label_values=None, ignore_label=None, connectivity: int = 6, device=None) -> dict:
    """The overlap table of the components of ``truth`` (values mapped to classes) and of ``pred`` (class indices), the voxels whose
    truth is ignored left out, with what the scores need of the components that occur in it - int64 arrays throughout:
    ``a``, ``b``, ``count`` (the table); ``truth_roots`` / ``pred_roots`` (ascending), their ``truth_classes`` / ``pred_classes`` (the
    class byte at the root: 254 for a truth value that is no class, 255 for a prediction that fits no byte) and ``truth_sizes`` /
    ``pred_sizes``; ``shape`` (Z, Y, X); ``classes`` (the class indices asked for); ``runs`` (the key runs along x)."""
    if tuple(pred.shape) != tuple(truth.shape):
        raise ValueError(f"prediction shape {tuple(pred.shape)} and ground-truth shape {tuple(truth.shape)} differ")
    class_list = _class_list(classes)
    zyx = lv.zyx(tuple(pred.shape))
    n = zyx[0] * zyx[1] * zyx[2]
    if int(connectivity) not in (6, 18, 26) or n >= co.VOXEL_LIMIT:
        raise ValueError(f"connectivity {connectivity} on a volume of {n} voxels: connectivity is 6, 18 or 26 and components need fewer than 2^31 voxels")
    t, lut = ev.class_bytes(truth, label_values, ignore_label)
    p = lv.lenient_u8(pred)
    device = lv.pick_device(device, pred, truth)
    if device is None:
        tc = lut[np.ascontiguousarray(lv.to_host(t))].reshape(zyx)
        ph = np.ascontiguousarray(lv.to_host(p)).reshape(zyx)
        a, b = co.label_components(tc, int(connectivity), device="cpu"), co.label_components(ph, int(connectivity), device="cpu")
        skip = (tc == ev.IGNORE) if (lut == ev.IGNORE).any() else None
        ta, tb, count = table_host(a.reshape(-1), b.reshape(-1), None if skip is None else skip.reshape(-1))
        runs = count_runs_host(a, b, skip, zyx[2])
        truth_roots, pred_roots = np.unique(ta), np.unique(tb)
        truth_classes, pred_classes = tc.reshape(-1)[truth_roots].astype(np.int64), ph.reshape(-1)[pred_roots].astype(np.int64)
    else:
        import torch
        from .. import _lib
        # both root volumes, the class bytes and their int64 index, the skip mask, the labelling's workspace, the uploads
        need = 8 * n + 9 * n + n + int(_lib.lib.vs_components_workspace_bytes(*zyx)) + sum(n for x in (t, p) if not lv.is_resident(x, device))
        lv.require_memory(device, need, f"the object overlaps of a {tuple(pred.shape)} volume")
        td, pd = lv.aligned_u8(t, device), lv.aligned_u8(p, device)
        tc = lv.aligned_u8(torch.from_numpy(lut).to(device)[td.to(torch.int64)], device)
        a, b = co.label_device(tc, zyx, connectivity), co.label_device(pd, zyx, connectivity)
        skip = (tc == ev.IGNORE).to(torch.uint8) if (lut == ev.IGNORE).any() else None
        runs = runs_device(a, b, skip, zyx[2])
        ta, tb, count = table_device(a, b, skip, zyx[2])
        truth_roots, pred_roots = np.unique(ta), np.unique(tb)
        truth_classes = tc[torch.from_numpy(truth_roots).to(device)].cpu().numpy().astype(np.int64)
        pred_classes = pd[torch.from_numpy(pred_roots).to(device)].cpu().numpy().astype(np.int64)
    truth_sizes, pred_sizes = _group_sums(truth_roots, ta, count), _group_sums(pred_roots, tb, count)
    return dict(a=ta, b=tb, count=count, truth_roots=truth_roots, truth_classes=truth_classes, truth_sizes=truth_sizes, pred_roots=pred_roots,
                pred_classes=pred_classes, pred_sizes=pred_sizes, shape=np.array(zyx, dtype=np.int64),
                classes=np.array(class_list, dtype=np.int64), runs=int(runs))


def _group_sums(roots: np.ndarray, members: np.ndarray, count: np.ndarray) -> np.ndarray:
    """per root (ascending, every member among them) the int64 sum of ``count`` over the table rows that name it"""
    sums = np.zeros(len(roots), dtype=np.int64)
    np.add.at(sums, np.searchsorted(roots, members), count)
    return sums


# ---- the figures -------------------------------------------------------------------------------------------------------------------
def _thresholds(iou) -> list[float]:
    values = [float(iou)] if np.isscalar(iou) else [float(t) for t in iou]
    if not values or any(not 0.5 <= t < 1.0 for t in values):
        raise ValueError(f"evaluation_object_iou {iou!r}: one threshold or a list of them, each in [0.5, 1)")
    return values


def _ratio(num: float, den: float) -> float:
    return float(num) / float(den) if den else float("nan")


def object_scores_from_overlaps(overlaps: dict, iou=0.5, min_voxels: int = 1, min_overlap: int = 1, background: bool = False) -> dict:
    """The figures of ``object_overlaps``' output, float64 from its integers alone (pure host code).  Returns ``{"settings",
    "classes": [per class: class, true_objects, predicted_objects, splits, merges, thresholds: [per threshold: iou_threshold, tp, fp,
    fn, precision, recall, f1, sq, pq]], "means": [per threshold: the means of precision, recall, f1, sq and pq over the classes that
    have an object on either side], "partition": {voxels, vi_split, vi_merge, vi, adapted_rand_error, rand_precision,
    rand_recall}, "matches": [one row per true object, then the predicted objects no true object lists as matched]}``.  A class
    without objects on either side has NaN for every figure and is left out of the means."""
    thresholds = _thresholds(iou)
    min_voxels, min_overlap = int(min_voxels), int(min_overlap)
    if min_voxels < 1 or min_overlap < 1:
        raise ValueError("evaluation_object_min_voxels and evaluation_object_min_overlap must be at least 1")
    ta, tb, count = (np.asarray(overlaps[k], dtype=np.int64) for k in ("a", "b", "count"))
    t_roots, p_roots = np.asarray(overlaps["truth_roots"], dtype=np.int64), np.asarray(overlaps["pred_roots"], dtype=np.int64)
    t_class, p_class = np.asarray(overlaps["truth_classes"], dtype=np.int64), np.asarray(overlaps["pred_classes"], dtype=np.int64)
    t_size, p_size = np.asarray(overlaps["truth_sizes"], dtype=np.int64), np.asarray(overlaps["pred_sizes"], dtype=np.int64)
    zyx = tuple(int(s) for s in overlaps["shape"])
    class_list = [int(c) for c in overlaps["classes"]]
    scored = [c for c in class_list if c != 0 or background]
    ti, pi = np.searchsorted(t_roots, ta), np.searchsorted(p_roots, tb)         # the table's rows as indices into the components
    t_object = np.isin(t_class, scored) & (t_size >= min_voxels)
    p_object = np.isin(p_class, scored) & (p_size >= min_voxels)
    # the pairs of two objects of one class, in table order (by true root, then predicted root)
    pair = t_object[ti] & p_object[pi] & (t_class[ti] == p_class[pi])
    pt, pp, pn = ti[pair], pi[pair], count[pair]
    pair_iou = pn.astype(np.float64) / (t_size[pt] + p_size[pp] - pn).astype(np.float64)
    touching = pn >= min_overlap
    t_partners = np.bincount(pt[touching], minlength=len(t_roots))
    p_partners = np.bincount(pp[touching], minlength=len(p_roots))

    # per true object its best partner: the largest overlap, the lower predicted root on a tie (the table is sorted by it)
    best = np.full(len(t_roots), -1, dtype=np.int64)
    order = np.lexsort((pp, -pn, pt))
    first_of, at = np.unique(pt[order], return_index=True)               # the first row of every true object's stretch
    best[first_of] = order[at]
    per_class, listed = [], np.zeros(len(p_roots), dtype=bool)
    for c in class_list:
        mine_t, mine_p = t_object & (t_class == c), p_object & (p_class == c)
        nt, npred = int(mine_t.sum()), int(mine_p.sum())
        empty = c not in scored or nt + npred == 0
        entry = dict(index=c, true_objects=nt if c in scored else 0, predicted_objects=npred if c in scored else 0,
                     splits=float("nan") if empty else int((t_partners[mine_t] >= 2).sum()),
                     merges=float("nan") if empty else int((p_partners[mine_p] >= 2).sum()), thresholds=[])
        of_class = t_class[pt] == c
        for t in thresholds:
            if empty:
                entry["thresholds"].append(dict(iou_threshold=t, tp=0, fp=0, fn=0, **{k: float("nan") for k in ("precision", "recall", "f1", "sq", "pq")}))
                continue
            hit = of_class & (pair_iou > t)
            tp = int(hit.sum())
            fp, fn = npred - tp, nt - tp
            total = math.fsum(pair_iou[hit].tolist())
            entry["thresholds"].append(dict(iou_threshold=t, tp=tp, fp=fp, fn=fn, precision=_ratio(tp, tp + fp), recall=_ratio(tp, tp + fn),
                                            f1=_ratio(2 * tp, 2 * tp + fp + fn), sq=_ratio(total, tp), pq=_ratio(total, tp + 0.5 * fp + 0.5 * fn)))
        per_class.append(entry)
    means = []
    for k, t in enumerate(thresholds):
        row = dict(iou_threshold=t)
        for name in ("precision", "recall", "f1", "sq", "pq"):
            values = [e["thresholds"][k][name] for e in per_class if e["index"] in scored and e["true_objects"] + e["predicted_objects"] > 0]
            values = [v for v in values if not math.isnan(v)]
            row[name] = math.fsum(values) / len(values) if values else float("nan")
        means.append(row)

    # the match list: every true object, then the predicted objects none of them lists as matched
    matches = []
    coords = lambda root: tuple(int(c) for c in np.unravel_index(int(root), zyx))          # noqa: E731
    for i in np.flatnonzero(t_object):
        row = dict(kind="truth", index=int(t_class[i]), root=coords(t_roots[i]), voxels=int(t_size[i]), predicted_root=None, predicted_voxels=None,
                   overlap=0, iou=0.0, matched=False, overlapping_predicted=int(t_partners[i]))
        if best[i] >= 0:
            j = pp[best[i]]
            row.update(predicted_root=coords(p_roots[j]), predicted_voxels=int(p_size[j]), overlap=int(pn[best[i]]), iou=float(pair_iou[best[i]]),
                       matched=bool(pair_iou[best[i]] > thresholds[0]))
            if row["matched"]:
                listed[j] = True
        matches.append(row)
    for j in np.flatnonzero(p_object & ~listed):
        matches.append(dict(kind="predicted", index=int(p_class[j]), root=None, voxels=None, predicted_root=coords(p_roots[j]),
                            predicted_voxels=int(p_size[j]), overlap=None, iou=None, matched=False, overlapping_predicted=None))

    settings = dict(iou=thresholds, min_voxels=min_voxels, min_overlap=min_overlap, background=bool(background))
    return dict(settings=settings, classes=per_class, means=means, partition=partition_scores(ta, tb, count), matches=matches,
                shape=list(zyx), table_rows=int(len(count)), runs=int(overlaps.get("runs", -1)))


def _sum_of_squares(x: np.ndarray) -> int:
    """the exact sum of x^2 as a Python integer, 0 <= x < 2^31: with x = 2^16 h + l the three int64 sums of h^2, h l and l^2 stay below
    2^62 for any table a volume below 2^31 voxels can give (their entries sum to the voxel count at most)"""
    h, l = x >> 16, x & 0xFFFF
    return (int((h * h).sum()) << 32) + (int((h * l).sum()) << 17) + int((l * l).sum())


def partition_scores(a, b, count) -> dict:
    """variation of information (bits) and the adapted Rand error of the two partitions a table describes; the table sorted by key"""
    a, b, count = (np.asarray(x, dtype=np.int64) for x in (a, b, count))
    total = int(count.sum())
    if total == 0:
        nan = float("nan")
        return dict(voxels=0, vi_split=nan, vi_merge=nan, vi=nan, adapted_rand_error=nan, rand_precision=nan, rand_recall=nan)
    a_roots, a_index = np.unique(a, return_inverse=True)
    b_roots, b_index = np.unique(b, return_inverse=True)
    a_sum, b_sum = _group_sums(a_roots, a, count), _group_sums(b_roots, b, count)
    n = count.astype(np.float64)
    split = math.fsum((-(n / total) * np.log2(n / a_sum[a_index].astype(np.float64))).tolist())       # H(P | T)
    merge = math.fsum((-(n / total) * np.log2(n / b_sum[b_index].astype(np.float64))).tolist())       # H(T | P)
    both, sum_a, sum_b = _sum_of_squares(count), _sum_of_squares(a_sum), _sum_of_squares(b_sum)
    precision, recall = both / sum_b, both / sum_a
    return dict(voxels=total, vi_split=split + 0.0, vi_merge=merge + 0.0, vi=split + merge + 0.0,
                adapted_rand_error=1.0 - 2.0 * precision * recall / (precision + recall), rand_precision=precision, rand_recall=recall)


# ---- reporting ---------------------------------------------------------------------------------------------------------------------
_FIGURES = ("precision", "recall", "f1", "sq", "pq")
MATCH_COLUMNS = ("class", "label_value", "root_z", "root_y", "root_x", "voxels", "predicted_root_z", "predicted_root_y", "predicted_root_x",
                 "predicted_voxels", "overlap", "iou", "matched", "overlapping_predicted")
SCORE_COLUMNS = ("class", "label_value", "iou_threshold", "true_objects", "predicted_objects", "tp", "fp", "fn") + _FIGURES + ("splits", "merges")


def _values(scores: dict, label_values):
    indices = [e["index"] for e in scores["classes"]]
    values = {} if label_values is None else {i: int(v) for i, v in enumerate(label_values)}
    return {i: values.get(i, i if label_values is None else None) for i in indices}


def object_score_table(scores: dict, label_values=None) -> str:
    """the per-class table and the partition scores as text, for the log"""
    values = _values(scores, label_values)
    lines = [f"{'class':>5} {'value':>6} {'iou >':>6} {'true':>8} {'pred':>8} {'tp':>8} {'fp':>8} {'fn':>8} {'precision':>9} {'recall':>8} {'f1':>8} "
             f"{'sq':>8} {'pq':>8} {'splits':>7} {'merges':>7}"]
    for e in scores["classes"]:
        for row in e["thresholds"]:
            lines.append(f"{e['index']:>5} {values[e['index']]!s:>6} {row['iou_threshold']:>6g} {e['true_objects']:>8} {e['predicted_objects']:>8} "
                         f"{row['tp']:>8} {row['fp']:>8} {row['fn']:>8} {row['precision']:>9.5f} {row['recall']:>8.5f} {row['f1']:>8.5f} {row['sq']:>8.5f} "
                         f"{row['pq']:>8.5f} {e['splits']!s:>7} {e['merges']!s:>7}")
    for row in scores["means"]:
        lines.append(f"mean over the classes with objects, iou > {row['iou_threshold']:g}: precision {row['precision']:.5f}, recall {row['recall']:.5f}, "
                     f"f1 {row['f1']:.5f}, sq {row['sq']:.5f}, pq {row['pq']:.5f}")
    p = scores["partition"]
    lines.append(f"partitions of {p['voxels']} voxels: variation of information {p['vi']:.5f} bits (split {p['vi_split']:.5f}, merge {p['vi_merge']:.5f}), "
                 f"adapted Rand error {p['adapted_rand_error']:.5f}")
    return "\n".join(lines)


def json_ready(x):
    if isinstance(x, dict):
        return {k: json_ready(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [json_ready(v) for v in x]
    if isinstance(x, (float, np.floating)):
        return lv.json_number(x)
    if isinstance(x, np.integer):
        return int(x)
    return x


def write_object_scores(stem, scores: dict, label_values=None) -> list[Path]:
    """``<stem>_object_scores.csv`` (one row per class and threshold, then a ``mean`` row per threshold), ``<stem>_object_scores.json``
    (the settings, the per-class figures, the means and the partition scores; NaN is written as null) and ``<stem>_object_matches.csv``
    (one row per true object: where it is, its size, the predicted object of its class it overlaps most - the lower root on a tie
    -, that overlap and its IoU, whether the two match at the first threshold, and how many predicted objects overlap it; then one
    row per predicted object that no true object lists as matched, its truth columns empty)."""
    stem = str(stem)
    values = _values(scores, label_values)
    written = [Path(stem + "_object_scores.csv"), Path(stem + "_object_scores.json"), Path(stem + "_object_matches.csv")]
    blank = lambda x: "" if x is None else x                             # noqa: E731
    number = lambda x: repr(float(x))                                    # noqa: E731
    with open(written[0], "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(SCORE_COLUMNS)
        for e in scores["classes"]:
            for row in e["thresholds"]:
                w.writerow([e["index"], blank(values[e["index"]]), number(row["iou_threshold"]), e["true_objects"], e["predicted_objects"], row["tp"],
                            row["fp"], row["fn"]] + [number(row[k]) for k in _FIGURES] + [e["splits"], e["merges"]])
        for row in scores["means"]:
            w.writerow(["mean", "", number(row["iou_threshold"]), "", "", "", "", ""] + [number(row[k]) for k in _FIGURES] + ["", ""])
    doc = {k: scores[k] for k in ("settings", "shape", "table_rows", "runs", "classes", "means", "partition")}
    doc["classes"] = [dict(e, label_value=values[e["index"]]) for e in doc["classes"]]
    with open(written[1], "w") as f:
        json.dump(json_ready(doc), f, indent=1)
    with open(written[2], "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(MATCH_COLUMNS)
        for m in scores["matches"]:
            root, proot = m["root"] or ("", "", ""), m["predicted_root"] or ("", "", "")
            w.writerow([m["index"], blank(values.get(m["index"])), *root, blank(m["voxels"]), *proot, blank(m["predicted_voxels"]), blank(m["overlap"]),
                        "" if m["iou"] is None else number(m["iou"]), int(m["matched"]), blank(m["overlapping_predicted"])])
    return written


# ---- settings and the whole evaluation ------------------------------------------------------------------------------------------------
def object_scores_asked(settings) -> bool:
    """whether ``evaluation_object_scores`` is set - asked before the other keys are read, so that an evaluation that does not want
    object scores never fails over one of them"""
    return bool(getattr(settings, "evaluation_object_scores", False))


def object_settings(settings) -> dict:
    """the optional predict-settings keys ``evaluation_object_scores`` (as ``active``), ``evaluation_object_iou`` (a threshold or a list,
    each in [0.5, 1); default 0.5), ``evaluation_object_min_voxels`` (1), ``evaluation_object_min_overlap`` (1),
    ``evaluation_object_background`` (False) and ``evaluation_object_connectivity`` (default: ``postprocess_connectivity`` where that
    is set, else 6) as arguments"""
    connectivity = int(getattr(settings, "evaluation_object_connectivity", None) or getattr(settings, "postprocess_connectivity", None) or 6)
    if connectivity not in (6, 18, 26):
        raise ValueError(f"evaluation_object_connectivity {connectivity}: it is 6, 18 or 26")
    iou = getattr(settings, "evaluation_object_iou", None)
    min_voxels, min_overlap = getattr(settings, "evaluation_object_min_voxels", None), getattr(settings, "evaluation_object_min_overlap", None)
    out = dict(active=object_scores_asked(settings), connectivity=connectivity, iou=_thresholds(0.5 if iou is None else iou),
               min_voxels=1 if min_voxels is None else int(min_voxels), min_overlap=1 if min_overlap is None else int(min_overlap),
               background=bool(getattr(settings, "evaluation_object_background", False)))
    if out["min_voxels"] < 1 or out["min_overlap"] < 1:
        raise ValueError("evaluation_object_min_voxels and evaluation_object_min_overlap must be at least 1")
    return out


def evaluate_objects(pred, truth, classes, settings, *, label_values=None, ignore_label=None, device=None, stem=None):
    """What the evaluate command and ``evaluate_volume`` do with ``evaluation_object_scores: true``: the overlap table, the figures,
    the table in the log and, with ``stem``, the three files.  Returns (scores, overlaps)."""
    import logging
    o = object_settings(settings)
    overlaps = object_overlaps(pred, truth, classes, label_values=label_values, ignore_label=ignore_label, connectivity=o["connectivity"], device=device)
    scores = object_scores_from_overlaps(overlaps, o["iou"], o["min_voxels"], o["min_overlap"], o["background"])
    scores["settings"]["connectivity"] = o["connectivity"]
    logging.info("Object scores against the label volume:\n" + object_score_table(scores, label_values))
    if stem is not None:
        write_object_scores(stem, scores, label_values)
    return scores, overlaps
