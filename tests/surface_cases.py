"""Restatements the surface-distance tests share (tests/test_surface_distance_host.py, tests/test_hip_surface_distance.py), NumPy
only: squared distance transforms by brute force and by dense per-axis minima, surfaces by and-ing six shifts, the scores from
explicit distance arrays - nothing from a histogram - and the small coherent volumes the tests score."""
import functools

import numpy as np

INF = 0xFFFFFFFF


def brute_d2(seeds):
    """uint32 squared distance to the nearest seed: the minimum over ALL seeds, in chunks of voxels"""
    seeds = np.asarray(seeds) != 0
    out = np.full(seeds.size, INF, dtype=np.uint32)
    pts = np.argwhere(seeds).astype(np.int64)
    if len(pts):
        vox = np.indices(seeds.shape).reshape(seeds.ndim, -1).T.astype(np.int64)
        chunk = max(1, (1 << 24) // len(pts))
        for a in range(0, len(vox), chunk):
            out[a:a + chunk] = ((vox[a:a + chunk, None, :] - pts[None, :, :]) ** 2).sum(2).min(1)
    return out.reshape(seeds.shape)


def minplus_d2(seeds):
    """the same by three dense per-axis minima out(p) = min over p' of f(p') + (p - p')^2 (int64, a large mark for "none")"""
    seeds = np.asarray(seeds) != 0
    big = np.int64(1) << 40
    d = np.where(seeds, np.int64(0), big)
    for axis in range(seeds.ndim):
        f = np.moveaxis(d, axis, 0)
        length = f.shape[0]
        off = (np.arange(length)[:, None] - np.arange(length)[None, :]).astype(np.int64) ** 2      # [p][p']
        d = np.moveaxis((f[None, ...] + off.reshape(length, length, *([1] * (f.ndim - 1)))).min(1), 0, axis)
    return np.where(d >= big, INF, d).astype(np.uint32)


def surface_np(mask):
    """voxels of the mask with a face neighbour outside it: pad with False, and the six shifts; an axis of length 1 is skipped"""
    m = np.asarray(mask, dtype=bool)
    p = np.pad(m, 1, constant_values=False)
    core = tuple(slice(1, -1) for _ in range(m.ndim))
    interior = np.ones_like(m)
    for axis in range(m.ndim):
        if m.shape[axis] == 1:
            continue
        for shift in (0, 2):
            sl = list(core)
            sl[axis] = slice(shift, shift + m.shape[axis])
            interior &= p[tuple(sl)]
    return m & ~interior


def class_masks(pred, truth_classes, cls, ignored=None):
    """(A, B) of one class: truth-class and predicted-class voxels, minus the ignored ones"""
    keep = np.ones(np.shape(pred), dtype=bool) if ignored is None else ~np.asarray(ignored)
    return (np.asarray(truth_classes) == cls) & keep, (np.asarray(pred) == cls) & keep


def directed_d2(pred, truth_classes, cls, ignored=None, d2=minplus_d2):
    """(d2 of every truth-surface voxel to the predicted surface, the other way round) as flat uint32 arrays"""
    a, b = class_masks(pred, truth_classes, cls, ignored)
    sa, sb = surface_np(a), surface_np(b)
    return d2(sb)[sa], d2(sa)[sb]


def histograms_np(pred, truth_classes, classes, ignored=None, d2=minplus_d2):
    """what surface_distance_histograms returns: (K, 2, bins) trimmed of trailing all-zero bins, and the INF counts (K, 2)"""
    per = [directed_d2(pred, truth_classes, c, ignored, d2) for c in range(classes)]
    top = max([int(v[v != INF].max()) for pair in per for v in pair if (v != INF).any()] + [0])
    hists = np.zeros((classes, 2, top + 1), dtype=np.int64)
    inf = np.zeros((classes, 2), dtype=np.int64)
    for c, pair in enumerate(per):
        for d, v in enumerate(pair):
            inf[c, d] = int((v == INF).sum())
            hists[c, d] = np.bincount(v[v != INF].astype(np.int64), minlength=top + 1)
    return hists, inf


def brute_surface_scores(pred, truth_classes, classes, tolerance=1.0, voxel_size=1.0, ignored=None, d2=minplus_d2):
    """per-class figures from explicit distance arrays: np.percentile, np.mean, max; means over the classes present in either"""
    names = ("hausdorff", "hausdorff_95", "assd", "mean_distance_truth_to_pred", "mean_distance_pred_to_truth", "surface_dice")
    out = {n: [] for n in names + ("truth_surface_voxels", "predicted_surface_voxels", "truth_within_tolerance", "predicted_within_tolerance")}
    for c in range(classes):
        tp, pt = directed_d2(pred, truth_classes, c, ignored, d2)
        out["truth_surface_voxels"].append(int(tp.size))
        out["predicted_surface_voxels"].append(int(pt.size))
        if tp.size + pt.size == 0:
            figures = [float("nan")] * 6
            within = (0, 0)
        elif tp.size == 0 or pt.size == 0:
            figures = [float("inf")] * 5 + [0.0]
            within = (0, 0)
        else:
            dtp, dpt = voxel_size * np.sqrt(tp.astype(np.float64)), voxel_size * np.sqrt(pt.astype(np.float64))
            pooled = np.concatenate([dtp, dpt])
            within = (int((dtp <= tolerance).sum()), int((dpt <= tolerance).sum()))
            figures = [float(pooled.max()), float(np.percentile(pooled, 95)), float(np.mean(pooled)), float(np.mean(dtp)), float(np.mean(dpt)),
                       (within[0] + within[1]) / pooled.size]
        for n, v in zip(names, figures):
            out[n].append(v)
        out["truth_within_tolerance"].append(within[0])
        out["predicted_within_tolerance"].append(within[1])
    present = [c for c in range(classes) if out["truth_surface_voxels"][c] + out["predicted_surface_voxels"][c]]
    for n, m in (("hausdorff", "mean_hausdorff"), ("hausdorff_95", "mean_hausdorff_95"), ("assd", "mean_assd"), ("surface_dice", "mean_surface_dice")):
        out[m] = float(np.mean([out[n][c] for c in present])) if present else float("nan")
    return out


FLOAT_FIGURES = ("hausdorff", "hausdorff_95", "assd", "mean_distance_truth_to_pred", "mean_distance_pred_to_truth")
INTEGER_FIGURES = ("truth_surface_voxels", "predicted_surface_voxels", "truth_within_tolerance", "predicted_within_tolerance")


def assert_surface_scores_equal(s, b):
    """integers exactly; distances within rtol 1e-10 (float64 summation order over at most about 10^4 terms); surface Dice 1e-15"""
    for name in INTEGER_FIGURES:
        assert np.asarray(getattr(s, name)).tolist() == b[name], name
    for name in FLOAT_FIGURES:
        np.testing.assert_allclose(getattr(s, name), np.array(b[name]), rtol=1e-10, atol=0, equal_nan=True, err_msg=name)
    np.testing.assert_allclose(s.surface_dice, np.array(b["surface_dice"]), rtol=0, atol=1e-15, equal_nan=True)
    for name in ("mean_hausdorff", "mean_hausdorff_95", "mean_assd"):
        np.testing.assert_allclose(getattr(s, name), b[name], rtol=1e-10, atol=0, equal_nan=True, err_msg=name)
    np.testing.assert_allclose(s.mean_surface_dice, b["mean_surface_dice"], rtol=0, atol=1e-15, equal_nan=True)


# ---- volumes ---------------------------------------------------------------------------------------------------------------------
def _box_mean(field, r):
    """box average of half-width r along every axis by cumulative sums (edges: the window is cut at the volume's faces)"""
    for axis in range(field.ndim):
        f = np.moveaxis(field, axis, 0)
        c = np.concatenate([np.zeros((1,) + f.shape[1:]), np.cumsum(f, axis=0)])
        idx = np.arange(f.shape[0])
        lo, hi = np.maximum(idx - r, 0), np.minimum(idx + r + 1, f.shape[0])
        shape = (-1,) + (1,) * (f.ndim - 1)
        field = np.moveaxis((c[hi] - c[lo]) / (hi - lo).reshape(shape), 0, axis)
    return field


@functools.lru_cache(maxsize=None)
def coherent_pair(shape=(12, 24, 40), seed=0, flips=40):
    """(pred, truth) uint8 class indices 0..3 (read-only): truth = a smoothed random field cut at its quartiles, pred = truth shifted
    by one voxel along y with `flips` voxels set to other classes at fixed seeds"""
    rng = np.random.default_rng(seed)
    field = _box_mean(rng.standard_normal(shape), 2)
    truth = np.searchsorted(np.quantile(field, [0.25, 0.5, 0.75]), field).astype(np.uint8)
    pred = np.roll(truth, 1, axis=len(shape) - 2).copy()
    where = rng.choice(truth.size, flips, replace=False)
    pred.reshape(-1)[where] = (pred.reshape(-1)[where] + rng.integers(1, 4, flips)) % 4
    pred.setflags(write=False)
    truth.setflags(write=False)
    return pred, truth


@functools.lru_cache(maxsize=None)
def coherent_reference(shape=(12, 24, 40), seed=0):
    """(hists, inf) of the coherent pair by minplus_d2, computed once and shared (read-only)"""
    pred, truth = coherent_pair(shape, seed)
    hists, inf = histograms_np(pred, truth, 4)
    hists.setflags(write=False)
    inf.setflags(write=False)
    return hists, inf
