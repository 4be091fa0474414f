"""Scoring a predicted label volume against a labelled one.

``confusion_matrix`` counts (truth class, predicted class) pairs - one HIP sweep over the two uint8 volumes
(vs_confusion_matrix, csrc/evaluate.hip) where there is a GPU, ``torch.bincount`` on the device above the kernel's 16
classes, ``np.bincount`` on a host without one; the three give the same integers.  ``scores_from_confusion`` turns the
integers into per-class Dice / IoU / precision / recall in float64, ``truth_label_values`` is the rule that pairs a class
index with a ground-truth value, and ``write_scores`` puts the figures on disk."""
from __future__ import annotations

import csv
import json
import re
from dataclasses import dataclass
from pathlib import Path

import numpy as np

from . import label_volume as lv

KERNEL_MAX_CLASSES = 16       # vs_confusion_matrix: the pair code t * K + p is one byte
MAX_CLASSES = 254             # class bytes 254 / 255 are the table's "invalid" / "ignore" marks
IGNORE, INVALID = 255, 254


@dataclass
class SegmentationScores:
    """Figures of one confusion matrix (row = truth class, column = predicted class), float64 from exact integers."""
    confusion: np.ndarray          # (K, K) int64
    truth_voxels: np.ndarray       # (K,) int64: row sums
    predicted_voxels: np.ndarray   # (K,) int64: column sums
    true_positives: np.ndarray     # (K,) int64: the diagonal
    dice: np.ndarray               # 2 TP / (T + P)
    iou: np.ndarray                # TP / (T + P - TP)
    precision: np.ndarray          # TP / P
    recall: np.ndarray             # TP / T
    accuracy: float                # sum(TP) / counted voxels
    mean_dice: float
    mean_iou: float

    @property
    def classes(self) -> int:
        return int(self.confusion.shape[0])


def scores_from_confusion(counts) -> SegmentationScores:
    """Per-class and mean scores of a (K, K) confusion matrix.

    Convention for absent classes: a class with no voxel in the truth AND none in the prediction has nothing to score - its
    Dice, IoU, precision and recall are NaN and it is left out of ``mean_dice`` / ``mean_iou``, which average over the classes
    present in truth or prediction.  A class absent from the truth but predicted somewhere scores Dice = IoU = 0 and stays
    in the means (precision 0, recall NaN); one present in the truth and never predicted likewise (recall 0, precision NaN).
    The trainer's ``MeanIoU`` (data/losses.py, the reference's metric) differs: it scores an absent class as 0 / 1e-8 = 0
    and divides by the full class count, so the two agree only when every class is present."""
    c = np.asarray(counts)
    if c.ndim != 2 or c.shape[0] != c.shape[1]:
        raise ValueError(f"expected a square (K, K) confusion matrix, got shape {c.shape} (per-slice counts: sum over axis 0, or dice_per_slab)")
    c = c.astype(np.int64)
    t, p, tp = c.sum(1), c.sum(0), np.diagonal(c).copy()
    tf, pf, tpf = t.astype(np.float64), p.astype(np.float64), tp.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        dice = 2.0 * tpf / (tf + pf)
        iou = tpf / (tf + pf - tpf)
        precision = tpf / pf
        recall = tpf / tf
        total = float(c.sum())
        accuracy = float(tpf.sum() / total) if total else float("nan")
    present = (t + p) > 0
    mean_dice = float(dice[present].mean()) if present.any() else float("nan")
    mean_iou = float(iou[present].mean()) if present.any() else float("nan")
    return SegmentationScores(c, t, p, tp, dice, iou, precision, recall, accuracy, mean_dice, mean_iou)


def dice_per_slab(counts) -> np.ndarray:
    """(S, K) Dice of each class in each slab of per-slice counts (S, K, K); NaN where a class is absent from both."""
    c = np.asarray(counts).astype(np.float64)
    if c.ndim != 3:
        raise ValueError(f"expected (S, K, K) per-slice counts, got shape {c.shape}")
    with np.errstate(invalid="ignore", divide="ignore"):
        return 2.0 * np.diagonal(c, axis1=1, axis2=2) / (c.sum(2) + c.sum(1))


_LABEL_VAL = re.compile(r"^label_val_(-?\d+)$")


def truth_label_values(label_codes, truth, classes: int, ignore_label=None, label_values=None) -> np.ndarray:
    """The ground-truth value of every class index, ascending: class ``i`` is the ``i``-th ground-truth value in ascending
    order, which is what TrainingDataSlicer._preprocess_labels / _fix_label_classes did to the training labels.

    An explicit ``label_values`` wins.  Otherwise checkpoint label codes of the ``label_val_<v>`` form (the slicer's own) give the
    values; otherwise the ascending unique values of ``truth`` without ``ignore_label``.  More than ``classes`` values is an error."""
    if label_values is not None:
        values = np.asarray(list(label_values), dtype=np.int64)
        if len(np.unique(values)) != len(values):
            raise ValueError(f"label_values {values.tolist()} repeats a value")
    else:
        values = None
        if label_codes:
            names = list(label_codes.keys()) + list(label_codes.values()) if isinstance(label_codes, dict) else list(label_codes)
            found = [int(m.group(1)) for m in (_LABEL_VAL.match(s) for s in names if isinstance(s, str)) if m]
            if found:
                values = np.unique(np.asarray(found, dtype=np.int64))
        if values is None:
            values = np.unique(lv.to_host(truth)).astype(np.int64)
            if ignore_label is not None:
                values = values[values != int(ignore_label)]
    if len(values) > classes:
        raise ValueError(f"the ground truth has {len(values)} label values {values.tolist()[:20]} but the model predicts {classes} classes")
    return values


# ---- counting ------------------------------------------------------------------------------------------------------------
def truth_table(classes: int, label_values, ignore_label) -> np.ndarray:
    """raw ground-truth byte -> class index (255 ignore, 254 invalid)"""
    lut = np.full(256, INVALID, dtype=np.uint8)
    values = np.arange(classes) if label_values is None else np.asarray(label_values, dtype=np.int64)
    for i, v in enumerate(values):
        if 0 <= int(v) <= 255:
            lut[int(v)] = i
    if ignore_label is not None and 0 <= int(ignore_label) <= 255:
        lut[int(ignore_label)] = IGNORE
    return lut


def wide_truth_to_classes(truth: np.ndarray, classes: int, label_values, ignore_label) -> np.ndarray:
    """ground truth of a wider integer dtype -> uint8 class indices (255 ignore, 254 invalid) on the host"""
    values = np.arange(classes, dtype=np.int64) if label_values is None else np.asarray(label_values, dtype=np.int64)
    order = np.argsort(values, kind="stable")
    sorted_values = values[order]
    flat = truth.reshape(-1).astype(np.int64, copy=False)
    out = np.full(flat.shape, INVALID, dtype=np.uint8)
    if len(values):
        pos = np.clip(np.searchsorted(sorted_values, flat), 0, len(values) - 1)
        hit = sorted_values[pos] == flat
        out[hit] = order[pos[hit]].astype(np.uint8)
    if ignore_label is not None:
        out[flat == int(ignore_label)] = IGNORE
    return out.reshape(truth.shape)


def class_bytes(labels, label_values, ignore_label):
    """(uint8 volume - host array or device tensor -, 256-entry table byte -> class with 255 = ignore, 254 = no class): a uint8 volume
    as it came with the table that maps it, a wider one mapped on the host with the identity table.  Without ``label_values`` class
    ``i`` is the value ``i``.  What the surface distances and the object scores label their ground truth with."""
    if lv.is_u8(labels):
        lut = np.arange(256, dtype=np.uint8)
        lut[254:] = INVALID
        if label_values is not None:
            lut = truth_table(len(label_values), label_values, None)
        if ignore_label is not None and 0 <= int(ignore_label) <= 255:
            lut[int(ignore_label)] = IGNORE
        return labels, lut
    host = lv.to_host(labels)
    if host.dtype == np.bool_:
        host = host.astype(np.uint8)
    if not np.issubdtype(host.dtype, np.integer):
        raise TypeError(f"expected an integer label volume, got {host.dtype}")
    return wide_truth_to_classes(host, 254, label_values, ignore_label), np.arange(256, dtype=np.uint8)


def _count_numpy(t: np.ndarray, p: np.ndarray, lut: np.ndarray, classes: int, nslabs: int):
    k2 = classes * classes
    counts = np.zeros((nslabs, classes, classes), dtype=np.int64)
    dropped = np.zeros((nslabs, 2), dtype=np.int64)
    t, p = t.reshape(nslabs, -1), p.reshape(nslabs, -1)
    for s in range(nslabs):
        tc = lut[t[s]].astype(np.int64)
        ps = p[s].astype(np.int64)
        ignored = tc == IGNORE
        invalid = ~ignored & ((tc >= classes) | (ps >= classes))
        code = np.where(ignored, k2, np.where(invalid, k2 + 1, tc * classes + ps))
        b = np.bincount(code, minlength=k2 + 2)
        counts[s] = b[:k2].reshape(classes, classes)
        dropped[s] = b[k2:k2 + 2]
    return counts, dropped


def _count_torch(t, p, lut: np.ndarray, classes: int, nslabs: int):
    import torch

    k2 = classes * classes
    tc = torch.from_numpy(lut).to(t.device)[t.reshape(-1).long()].long()
    ps = p.reshape(-1).long()
    ignored = tc == IGNORE
    invalid = ~ignored & ((tc >= classes) | (ps >= classes))
    code = torch.where(ignored, k2, torch.where(invalid, k2 + 1, tc * classes + ps))
    slab = torch.arange(nslabs, device=t.device).repeat_interleave(t.numel() // nslabs)
    b = torch.bincount(code + slab * (k2 + 2), minlength=nslabs * (k2 + 2)).reshape(nslabs, k2 + 2).cpu().numpy().astype(np.int64)
    return b[:, :k2].reshape(nslabs, classes, classes).copy(), b[:, k2:].copy()


def _count_kernel(t, p, lut: np.ndarray, classes: int, nslabs: int):
    import torch
    from .. import _lib

    n = t.numel()
    lut_dev = torch.from_numpy(lut).to(t.device)
    counts = torch.empty((nslabs, classes, classes), dtype=torch.int64, device=t.device)
    dropped = torch.empty((nslabs, 2), dtype=torch.int64, device=t.device)
    with torch.cuda.device(t.device):
        _lib.check(_lib.lib.vs_confusion_matrix(_lib.ptr(t), _lib.ptr(p), n, classes, _lib.ptr(lut_dev), n // nslabs, _lib.ptr(counts),
                                                _lib.ptr(dropped), _lib.stream_ptr()))
    return counts.cpu().numpy(), dropped.cpu().numpy()


def _describe_invalid(truth_host, pred_host, classes, label_values, ignore_label) -> str:
    values = np.arange(classes) if label_values is None else np.asarray(label_values, dtype=np.int64)
    known = set(int(v) for v in values) | ({int(ignore_label)} if ignore_label is not None else set())
    bad_t = [int(v) for v in np.unique(truth_host) if int(v) not in known]
    bad_p = [int(v) for v in np.unique(pred_host) if not 0 <= int(v) < classes]
    parts = []
    if bad_t:
        parts.append(f"ground-truth values {bad_t[:20]} are none of the label values {values.tolist()}")
    if bad_p:
        parts.append(f"prediction values {bad_p[:20]} are outside 0..{classes - 1}")
    return "; ".join(parts)


def confusion_matrix(pred, truth, classes: int, *, label_values=None, ignore_label=None, per_slice: bool = False, device=None):
    """(counts, dropped) of a predicted label volume against ground truth of the same shape (host arrays or device tensors).

    counts: int64 (K, K), row = truth class, column = predicted class - or (S, K, K), one matrix per leading-axis slice,
    with ``per_slice``.  dropped: int64 (2,) or (S, 2) = [ignored, invalid] voxels, counted nowhere else.  Class ``i`` is the
    ground-truth value ``label_values[i]`` (default: ``i`` itself); ``ignore_label`` voxels are set aside.  A voxel whose truth is
    neither, or whose prediction is not below ``classes``, is invalid: that is never dropped silently - it raises ValueError
    with the count and the offending values.

    ``device``: where to count (default: the current GPU when there is one, else the host).  On a GPU up to 16 classes go through
    the HIP kernel, more through ``torch.bincount`` on the device; ``"cpu"`` or no GPU means ``np.bincount``.  All three return the
    same integers."""
    classes = int(classes)
    if not 1 <= classes <= MAX_CLASSES:
        raise ValueError(f"classes must be in 1..{MAX_CLASSES}, got {classes}")
    if tuple(pred.shape) != tuple(truth.shape):
        raise ValueError(f"prediction shape {tuple(pred.shape)} and ground-truth shape {tuple(truth.shape)} differ")
    shape = tuple(pred.shape)
    n = int(np.prod(shape)) if shape else 1
    if n == 0:
        raise ValueError("empty volumes")
    if per_slice and len(shape) < 2:
        raise ValueError("per_slice needs volumes with a leading slice axis")
    nslabs = shape[0] if per_slice else 1
    if label_values is not None and len(label_values) > classes:
        raise ValueError(f"{len(label_values)} label values for {classes} classes")

    device = lv.pick_device(device, pred, truth)

    # normal form of all three routes: uint8 truth + a 256-entry table, uint8 predictions
    if lv.is_u8(truth):
        t, lut = truth, truth_table(classes, label_values, ignore_label)
    else:
        th = lv.to_host(truth)
        if th.dtype != np.bool_ and not np.issubdtype(th.dtype, np.integer):
            raise TypeError(f"ground truth must be an integer label volume, got {th.dtype}")
        t = wide_truth_to_classes(th, classes, label_values, ignore_label)
        lut = np.arange(256, dtype=np.uint8)
        lut[classes:INVALID] = INVALID
    p = lv.lenient_u8(pred)

    if device is None:
        counts, dropped = _count_numpy(np.ascontiguousarray(lv.to_host(t)), np.ascontiguousarray(lv.to_host(p)), lut, classes, nslabs)
    else:
        td, pd = lv.aligned_u8(t, device), lv.aligned_u8(p, device)
        route = _count_kernel if classes <= KERNEL_MAX_CLASSES else _count_torch
        counts, dropped = route(td, pd, lut, classes, nslabs)
    invalid = int(dropped[:, 1].sum())
    if invalid:
        raise ValueError(f"{invalid} of {n} voxels cannot be scored: "
                         + _describe_invalid(lv.to_host(truth), lv.to_host(pred), classes, label_values, ignore_label))
    return (counts, dropped) if per_slice else (counts[0], dropped[0])


# ---- reporting -----------------------------------------------------------------------------------------------------------
_COLUMNS = ("truth_voxels", "predicted_voxels", "true_positives", "dice", "iou", "precision", "recall")


def score_table(scores: SegmentationScores, label_values=None) -> str:
    """the per-class table as text, for the log"""
    values = list(range(scores.classes)) if label_values is None else [int(v) for v in label_values]
    values += [""] * (scores.classes - len(values))
    lines = [f"{'class':>5} {'value':>6} {'truth':>12} {'predicted':>12} {'true pos':>12} {'dice':>8} {'iou':>8} {'precision':>9} {'recall':>8}"]
    for i in range(scores.classes):
        lines.append(f"{i:>5} {values[i]!s:>6} {int(scores.truth_voxels[i]):>12} {int(scores.predicted_voxels[i]):>12} "
                     f"{int(scores.true_positives[i]):>12} {scores.dice[i]:>8.5f} {scores.iou[i]:>8.5f} {scores.precision[i]:>9.5f} "
                     f"{scores.recall[i]:>8.5f}")
    lines.append(f"mean over the classes present: dice {scores.mean_dice:.5f}, iou {scores.mean_iou:.5f}; voxel accuracy {scores.accuracy:.5f}")
    return "\n".join(lines)


def write_scores(stem, scores: SegmentationScores, dropped, label_values=None, slab_dice=None) -> list[Path]:
    """``<stem>_scores.csv`` (one row per class: index, ground-truth value, the seven figures; then ``mean`` and ``accuracy``
    rows), ``<stem>_scores.json`` (the same, plus the confusion matrix and the dropped counts; NaN is written as null) and, given
    ``slab_dice`` (S, K), ``<stem>_scores_per_slice.csv`` (per leading-axis slice the Dice of each class)."""
    stem = str(stem)
    k = scores.classes
    values = list(range(k)) if label_values is None else [int(v) for v in label_values]
    values += [None] * (k - len(values))
    written = [Path(stem + "_scores.csv"), Path(stem + "_scores.json")]
    with open(written[0], "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(("class", "label_value") + _COLUMNS)
        for i in range(k):
            w.writerow([i, "" if values[i] is None else values[i], int(scores.truth_voxels[i]), int(scores.predicted_voxels[i]),
                        int(scores.true_positives[i]), repr(float(scores.dice[i])), repr(float(scores.iou[i])),
                        repr(float(scores.precision[i])), repr(float(scores.recall[i]))])
        w.writerow(["mean", "", "", "", "", repr(scores.mean_dice), repr(scores.mean_iou), "", ""])
        w.writerow(["accuracy", "", "", "", "", repr(scores.accuracy), "", "", ""])
    dropped = np.asarray(dropped).reshape(-1, 2).sum(0)
    doc = {"classes": [dict(index=i, label_value=values[i], truth_voxels=int(scores.truth_voxels[i]),
                            predicted_voxels=int(scores.predicted_voxels[i]), true_positives=int(scores.true_positives[i]),
                            dice=lv.json_number(scores.dice[i]), iou=lv.json_number(scores.iou[i]),
                            precision=lv.json_number(scores.precision[i]), recall=lv.json_number(scores.recall[i])) for i in range(k)],
           "mean_dice": lv.json_number(scores.mean_dice), "mean_iou": lv.json_number(scores.mean_iou), "accuracy": lv.json_number(scores.accuracy),
           "confusion_matrix": scores.confusion.tolist(), "dropped": {"ignored": int(dropped[0]), "invalid": int(dropped[1])}}
    with open(written[1], "w") as f:
        json.dump(doc, f, indent=1)
    if slab_dice is not None:
        written.append(Path(stem + "_scores_per_slice.csv"))
        with open(written[2], "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["slice"] + [f"dice_class_{i}" for i in range(k)])
            for s, row in enumerate(np.asarray(slab_dice)):
                w.writerow([s] + [repr(float(v)) for v in row])
    return written


def evaluate_label_volumes(pred, truth, classes: int, *, label_values=None, ignore_label=None, per_slice: bool = False, device=None):
    """count and score: (scores of the whole volume, dropped [ignored, invalid], per-slice Dice (S, K) or None)"""
    counts, dropped = confusion_matrix(pred, truth, classes, label_values=label_values, ignore_label=ignore_label,
                                       per_slice=per_slice, device=device)
    if per_slice:
        return scores_from_confusion(counts.sum(0)), dropped.sum(0), dice_per_slab(counts)
    return scores_from_confusion(counts), dropped, None
