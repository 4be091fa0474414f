"""Restatements the evaluation tests share (tests/test_evaluation_host.py, tests/test_hip_evaluation.py): every score from boolean
masks - nothing from a confusion matrix - and the confusion matrix itself from np.bincount."""
import numpy as np


def brute_scores(pred, truth, classes):
    """Per-class figures of class-index arrays, one boolean mask per class; means over the classes present in either."""
    out = dict(truth=[], pred=[], tp=[], dice=[], iou=[], precision=[], recall=[])
    for c in range(classes):
        t, p = truth == c, pred == c
        nt, npred, tp = int(t.sum()), int(p.sum()), int((t & p).sum())
        out["truth"].append(nt)
        out["pred"].append(npred)
        out["tp"].append(tp)
        out["dice"].append(2 * tp / (nt + npred) if nt + npred else float("nan"))
        out["iou"].append(tp / int((t | p).sum()) if nt + npred else float("nan"))
        out["precision"].append(tp / npred if npred else float("nan"))
        out["recall"].append(tp / nt if nt else float("nan"))
    present = [c for c in range(classes) if out["truth"][c] + out["pred"][c]]
    out["mean_dice"] = float(np.mean([out["dice"][c] for c in present]))
    out["mean_iou"] = float(np.mean([out["iou"][c] for c in present]))
    out["accuracy"] = float((pred == truth).mean())
    return out


def assert_scores_equal(s, b, tol=1e-12):
    assert s.truth_voxels.tolist() == b["truth"] and s.predicted_voxels.tolist() == b["pred"] and s.true_positives.tolist() == b["tp"]
    for name in ("dice", "iou", "precision", "recall"):
        np.testing.assert_allclose(getattr(s, name), np.array(b[name]), rtol=0, atol=tol, equal_nan=True, err_msg=name)
    for name in ("mean_dice", "mean_iou", "accuracy"):
        assert abs(getattr(s, name) - b[name]) <= tol, (name, getattr(s, name), b[name])


def random_pair(classes, shape=(6, 11, 13), seed=0):
    """(pred, truth) uint8 class indices: the prediction agrees with the truth on about 70 % of the voxels"""
    rng = np.random.default_rng(seed)
    truth = rng.integers(0, classes, shape).astype(np.uint8)
    pred = np.where(rng.random(shape) < 0.7, truth, rng.integers(0, classes, shape)).astype(np.uint8)
    return pred, truth


def bincount_confusion(truth, pred, classes, lut=None, slab_len=None):
    """vs_confusion_matrix restated: (counts [nslabs][K][K], dropped [nslabs][2] = ignored, invalid) of flat uint8 volumes.
    lut: 256 entries, raw truth byte -> class (255 ignore, 254 invalid); None: identity, every byte >= classes invalid."""
    truth, pred = np.asarray(truth).reshape(-1), np.asarray(pred).reshape(-1)
    n = truth.size
    slab_len = n if slab_len is None else slab_len
    nslabs = -(-n // slab_len)
    k2 = classes * classes
    tc = truth.astype(np.int64) if lut is None else np.asarray(lut)[truth].astype(np.int64)
    ignored = (tc == 255) if lut is not None else np.zeros(n, dtype=bool)
    invalid = ~ignored & ((tc >= classes) | (pred >= classes))
    code = np.where(ignored, k2, np.where(invalid, k2 + 1, tc * classes + pred))
    slab = np.arange(n, dtype=np.int64) // slab_len
    b = np.bincount(slab * (k2 + 2) + code, minlength=nslabs * (k2 + 2)).reshape(nslabs, k2 + 2)
    return b[:, :k2].reshape(nslabs, classes, classes).astype(np.int64), b[:, k2:].astype(np.int64)
