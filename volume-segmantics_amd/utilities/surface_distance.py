"""Surface-distance scores of a predicted label volume against a labelled one: Hausdorff distance (maximum and 95th percentile),
average symmetric surface distance and surface Dice at a tolerance, per class.

Definitions (unit voxels; ``voxel_size`` scales distances afterwards; under ``voxel_spacing: [sz, sy, sx]`` the squared distance is
the integer ``D = qz dz^2 + qy dy^2 + qx dx^2`` of ``label_volume.voxel_grid``, the histograms are indexed by ``D`` and a distance is
``unit * sqrt(D)`` - the surfaces do not depend on the spacing).  For class ``c``, ``A`` is the set of voxels whose truth
class is ``c`` and ``B`` the set whose predicted class is ``c``; a voxel whose truth is the ignore label is in neither.  The surface
``S(M)`` is every voxel of ``M`` with one of its six face neighbours not in ``M`` - a neighbour outside the volume is not in ``M``, an
axis of length 1 has no neighbours.  ``d2(v, S)`` is the squared Euclidean distance from ``v`` to the nearest voxel of ``S``, a uint32,
0xFFFFFFFF when ``S`` is empty.  Everything reported comes from two integer histograms per class - of ``d2(a, S(B))`` over ``a`` in
``S(A)`` (truth to prediction) and the other way round - so all routes give the same integers: four HIP kernels on a GPU
(csrc/surface.hip: vs_label_surface, vs_edt_squared, vs_surface_distance_histogram), ``scipy.ndimage.distance_transform_edt`` on a
host where scipy imports, a separable NumPy min-plus otherwise."""
from __future__ import annotations

import csv
import json
from dataclasses import dataclass
from pathlib import Path

import numpy as np

from . import evaluation as ev
from . import label_volume as lv

INF_D2 = 0xFFFFFFFF           # d2 of every voxel when there is no seed
EDT_LDS_MAX_AXIS = 512        # csrc/surface.hip kMaxLdsAxis: the longest y / z axis a workgroup's LDS tile holds
_DIRECTIONS = ("truth_to_pred", "pred_to_truth")
_zyx = lv.zyx                 # the shared shape rule under the name this module and its GPU tests have always used


# ---- shapes --------------------------------------------------------------------------------------------------------------------
def histogram_bins(shape) -> int:
    """(Z-1)^2 + (Y-1)^2 + (X-1)^2 + 2: every squared distance the volume can hold, then the bin of the 0xFFFFFFFF voxels"""
    z, y, x = _zyx(shape)
    most = (z - 1) ** 2 + (y - 1) ** 2 + (x - 1) ** 2
    if most >= INF_D2:
        raise ValueError(f"a volume of shape {tuple(shape)} can hold a squared distance of {most}, which does not fit below 2^32 - 1")
    return most + 2


# ---- host routes -----------------------------------------------------------------------------------------------------------------
def _surface_host(mask: np.ndarray) -> np.ndarray:
    m = np.asarray(mask, dtype=bool)
    interior = m.copy()
    for axis in range(m.ndim):
        if m.shape[axis] == 1:
            continue
        pad = [(0, 0)] * m.ndim
        pad[axis] = (1, 1)
        p = np.pad(m, pad, constant_values=False)
        lo = [slice(None)] * m.ndim
        hi = [slice(None)] * m.ndim
        lo[axis], hi[axis] = slice(0, -2), slice(2, None)
        interior &= p[tuple(lo)] & p[tuple(hi)]
    return m & ~interior


MAX_BINS = 1 << 28            # the longest histogram taken under voxel_spacing, where the bins follow the values present


def _minplus_axis(f: np.ndarray, axis: int, q: int = 1) -> np.ndarray:
    """out(p) = min over p' of f(p') + q (p - p')^2 along one axis, int64 with a large mark for "none" """
    f = np.moveaxis(f, axis, 0)
    length = f.shape[0]
    out = np.empty_like(f)
    pos = np.arange(length, dtype=np.int64)
    shape = (length,) + (1,) * (f.ndim - 1)
    for p in range(length):
        out[p] = (f + (q * (pos - p) ** 2).reshape(shape)).min(axis=0)
    return np.moveaxis(out, 0, axis)


def edt_host(seeds: np.ndarray, weights=lv.UNIT_WEIGHTS) -> np.ndarray:
    """the squared distances of a (Z, Y, X) volume; under ``weights`` the integers qz dz^2 + qy dy^2 + qx dx^2, q = w^2"""
    s = np.asarray(seeds) != 0
    if not s.any():
        return np.full(s.shape, INF_D2, dtype=np.uint32)
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    if ndimage is not None:
        if tuple(weights) == lv.UNIT_WEIGHTS:
            return np.rint(ndimage.distance_transform_edt(~s) ** 2).astype(np.uint32)
        return np.rint(ndimage.distance_transform_edt(~s, sampling=[float(w) for w in weights[3 - s.ndim:]]) ** 2).astype(np.uint32)
    big = np.int64(1) << 40
    d = np.where(s, np.int64(0), big)
    for axis in range(s.ndim - 1, -1, -1):
        d = _minplus_axis(d, axis, int(weights[3 - s.ndim + axis]) ** 2)
    return d.astype(np.uint32)


def _histogram_host(surface: np.ndarray, d2: np.ndarray, bins: int) -> np.ndarray:
    values = np.minimum(d2[surface != 0].astype(np.int64), bins - 1)
    return np.bincount(values, minlength=bins).astype(np.int64)


# ---- device routes ---------------------------------------------------------------------------------------------------------------
def edt_device(seeds_dev, zyx, d2_dev, workspace, weights=lv.UNIT_WEIGHTS):
    """vs_edt_squared on resident memory: ``seeds_dev`` n aligned uint8, ``d2_dev`` n int32 (uint32 bits), ``workspace`` a uint8 tensor of
    ``vs_edt_workspace_bytes`` bytes (empty where none is needed); vs_edt_squared_scaled under ``weights`` other than (1, 1, 1)"""
    import torch
    from .. import _lib
    with torch.cuda.device(seeds_dev.device):
        if tuple(weights) != lv.UNIT_WEIGHTS:
            _lib.check(_lib.lib.vs_edt_squared_scaled(_lib.ptr(seeds_dev), *zyx, *(int(w) for w in weights), _lib.ptr(d2_dev),
                                                      _lib.ptr(workspace) if workspace.numel() else None, workspace.numel(), _lib.stream_ptr()))
            return
        _lib.check(_lib.lib.vs_edt_squared(_lib.ptr(seeds_dev), *zyx, _lib.ptr(d2_dev), _lib.ptr(workspace) if workspace.numel() else None,
                                           workspace.numel(), _lib.stream_ptr()))


def _workspace(zyx, device):
    import torch
    from .. import _lib
    return torch.empty(int(_lib.lib.vs_edt_workspace_bytes(*zyx)), dtype=torch.uint8, device=device)


def _surface_device(labels_dev, lut_dev, cls, zyx, out_dev, count_dev=None):
    import torch
    from .. import _lib
    with torch.cuda.device(labels_dev.device):
        _lib.check(_lib.lib.vs_label_surface(_lib.ptr(labels_dev), _lib.ptr(lut_dev), int(cls), *zyx, _lib.ptr(out_dev), _lib.ptr(count_dev),
                                             _lib.stream_ptr()))


# ---- public: the pieces ------------------------------------------------------------------------------------------------------------
def squared_distance_transform(seeds, device=None, spacing=None) -> np.ndarray:
    """uint32 array of ``seeds.shape``: the exact squared Euclidean distance (unit voxels) from every voxel to the nearest non-zero
    voxel of ``seeds`` (a host array or a device tensor of one to three dimensions); 0xFFFFFFFF everywhere when there is none.
    ``spacing`` [sz, sy, sx] (the steps of the LAST three axes; default: unit voxels): the integers ``D = qz dz^2 + qy dy^2 + qx dx^2`` of
    ``label_volume.voxel_grid(spacing)``, so that a physical distance is ``unit * sqrt(D)``."""
    import torch
    shape = tuple(seeds.shape)
    zyx = _zyx(shape)
    histogram_bins(shape)        # raises when a squared distance would not fit
    weights, _ = lv.grid_of(spacing, zyx)
    device = lv.pick_device(device, seeds)
    if device is None:
        return edt_host(lv.to_host(seeds).reshape(zyx), weights).reshape(shape)
    n = int(np.prod(zyx))
    from .. import _lib
    lv.require_memory(device, 5 * n + int(_lib.lib.vs_edt_workspace_bytes(*zyx)), f"the distance transform of a {shape} volume")
    s = seeds if lv.is_tensor(seeds) else torch.from_numpy(np.ascontiguousarray(np.asarray(seeds) != 0).view(np.uint8))
    if s.dtype != torch.uint8:
        s = (s != 0).to(torch.uint8)
    s = lv.aligned_u8(s, device)
    d2 = torch.empty(n, dtype=torch.int32, device=device)
    edt_device(s, zyx, d2, _workspace(zyx, device), weights)
    return d2.cpu().numpy().view(np.uint32).reshape(shape)


def label_surface(labels, cls: int, *, label_values=None, ignore_label=None, device=None) -> np.ndarray:
    """uint8 mask of ``labels.shape``: 1 on the surface voxels of class ``cls``.  Class ``i`` is the value ``label_values[i]`` (default:
    ``i`` itself); voxels of ``ignore_label`` belong to no class."""
    import torch
    cls = int(cls)
    if not 0 <= cls <= 253:
        raise ValueError(f"class {cls}: classes are 0..253")
    shape = tuple(labels.shape)
    zyx = _zyx(shape)
    volume, lut = ev.class_bytes(labels, label_values, ignore_label)
    device = lv.pick_device(device, labels)
    if device is None:
        return _surface_host(lut[np.ascontiguousarray(lv.to_host(volume))] == cls).astype(np.uint8).reshape(shape)
    n = int(np.prod(zyx))
    lv.require_memory(device, 2 * n, f"the surface of a {shape} volume")
    v = lv.aligned_u8(volume, device)
    out = torch.empty(n, dtype=torch.uint8, device=device)
    _surface_device(v, torch.from_numpy(lut).to(device), cls, zyx, out)
    return out.cpu().numpy().reshape(shape)


def bins_present(largest: int) -> int:
    """the bins of a histogram under voxel_spacing: the largest finite value at the masked voxels, then its own bin, then the bin of
    the 0xFFFFFFFF voxels - not the bound of the shape, which the weights raise by up to 4096"""
    bins = int(largest) + 2
    if bins > MAX_BINS:
        raise ValueError(f"a histogram of {bins} bins: under voxel_spacing a histogram holds at most 2^28 = {MAX_BINS} - use a spacing with smaller "
                         f"integer weights")
    return bins


def _bins_host(surface: np.ndarray, d2: np.ndarray) -> int:
    at = d2[surface != 0]
    return bins_present(at[at != INF_D2].max() if (at != INF_D2).any() else 0)


def masked_max_device(mask, d2) -> int:
    """the largest value below 0xFFFFFFFF of ``d2`` (n int32, uint32 bits) at the voxels where ``mask`` (n uint8) is set; 0 where none"""
    import torch
    values = torch.where((mask != 0) & (d2 != -1), d2.to(torch.int64) & 0xFFFFFFFF, torch.zeros((), dtype=torch.int64, device=d2.device))
    return int(values.max())


def surface_distance_histograms(pred, truth, classes, *, label_values=None, ignore_label=None, device=None, spacing=None):
    """(hists, inf_counts) of a predicted label volume against ground truth of the same shape.

    ``classes``: the class count K (classes 0..K-1) or a sequence of class indices.  hists: int64 (K, 2, bins) - ``hists[i, 0, k]`` is
    the number of truth-surface voxels of class i at squared distance k from the predicted surface of that class, ``hists[i, 1, k]``
    the other way round - with the trailing bins that are zero everywhere trimmed.  inf_counts: int64 (K, 2), the surface voxels
    whose other surface is empty (d2 = 0xFFFFFFFF).  Truth values map to classes as in ``confusion_matrix``; the prediction holds
    class indices.  On a GPU the kernels run one class and one direction at a time over two masks, one d2 volume and the workspace.
    ``spacing`` [sz, sy, sx]: the histograms are indexed by ``D`` of ``label_volume.voxel_grid(spacing)`` - a distance is ``unit * sqrt(D)``;
    the surfaces themselves do not depend on it."""
    if tuple(pred.shape) != tuple(truth.shape):
        raise ValueError(f"prediction shape {tuple(pred.shape)} and ground-truth shape {tuple(truth.shape)} differ")
    shape = tuple(pred.shape)
    zyx = _zyx(shape)
    n = int(np.prod(zyx))
    weights, _ = lv.grid_of(spacing, zyx)
    scaled = weights != lv.UNIT_WEIGHTS
    bins = histogram_bins(shape)       # unit voxels: every squared distance of the shape has a bin; scaled: the bins follow the values present
    class_list = list(range(int(classes))) if np.isscalar(classes) else [int(c) for c in classes]
    if not class_list or min(class_list) < 0 or max(class_list) > 253:
        raise ValueError(f"classes must be 0..253, got {class_list[:20]}")
    t, lut = ev.class_bytes(truth, label_values, ignore_label)
    p = lv.lenient_u8(pred)
    device = lv.pick_device(device, pred, truth)
    full = {} if scaled else np.zeros((len(class_list), 2, bins), dtype=np.int64)     # scaled: (class, direction) -> its own bins

    if device is None:
        tc = lut[np.ascontiguousarray(lv.to_host(t))].reshape(zyx)
        ph = np.ascontiguousarray(lv.to_host(p)).reshape(zyx)
        ignored = tc == ev.IGNORE
        for i, c in enumerate(class_list):
            sa, sb = _surface_host(tc == c), _surface_host((ph == c) & ~ignored)
            if sa.any():
                d2 = edt_host(sb, weights)
                full[i, 0] = _histogram_host(sa, d2, _bins_host(sa, d2) if scaled else bins)
            if sb.any():
                d2 = edt_host(sa, weights)
                full[i, 1] = _histogram_host(sb, d2, _bins_host(sb, d2) if scaled else bins)
    else:
        import torch
        from .. import _lib
        work = int(_lib.lib.vs_edt_workspace_bytes(*zyx))
        need = 2 * n + 4 * n + work + (10 * n if scaled else 8 * bins) + (2 * n if ignore_label is not None else 0)
        need += sum(n for x in (t, p) if not lv.is_resident(x, device))
        lv.require_memory(device, need, f"surface distances of a {shape} volume")
        td, pd = lv.aligned_u8(t, device), lv.aligned_u8(p, device)
        lut_dev = torch.from_numpy(lut).to(device)
        if ignore_label is not None:       # a voxel whose truth is ignored is in no predicted class either
            ignored = _ignored_mask(td, lut)
            pd = torch.where(ignored, torch.full_like(pd, 255), pd)
            del ignored
        masks = [torch.empty(n, dtype=torch.uint8, device=device) for _ in range(2)]
        d2 = torch.empty(n, dtype=torch.int32, device=device)
        workspace = torch.empty(work, dtype=torch.uint8, device=device)
        hist = None if scaled else torch.empty(bins, dtype=torch.int64, device=device)
        counts = torch.empty(2, dtype=torch.int64, device=device)
        with torch.cuda.device(device):
            for i, c in enumerate(class_list):
                _surface_device(td, lut_dev, c, zyx, masks[0], counts[0:1])
                _surface_device(pd, None, c, zyx, masks[1], counts[1:2])
                for direction in range(2):
                    edt_device(masks[1 - direction], zyx, d2, workspace, weights)
                    if scaled:
                        bins = bins_present(masked_max_device(masks[direction], d2))
                        hist = torch.empty(bins, dtype=torch.int64, device=device)
                    _lib.check(_lib.lib.vs_surface_distance_histogram(_lib.ptr(masks[direction]), _lib.ptr(d2), n, bins, _lib.ptr(hist),
                                                                      _lib.stream_ptr()))
                    full[i, direction] = hist.cpu().numpy()
                held = [int(full[i, direction].sum()) for direction in range(2)]
                if held != counts.cpu().tolist():
                    raise RuntimeError(f"class {c}: the histograms hold {held} voxels, the surfaces {counts.cpu().tolist()}")
    if scaled:                  # to one array: the finite bins from the front, every histogram's last bin - its 0xFFFFFFFF voxels - into the last
        bins = max([len(h) for h in full.values()] + [2])
        padded = np.zeros((len(class_list), 2, bins), dtype=np.int64)
        for at, h in full.items():
            padded[at][:len(h) - 1] = h[:-1]
            padded[at][bins - 1] = h[-1]
        full = padded
    inf_counts = full[:, :, bins - 1].copy()
    finite = full[:, :, :bins - 1]
    used = np.flatnonzero(finite.any(axis=(0, 1)))
    keep = int(used[-1]) + 1 if len(used) else 1
    return np.ascontiguousarray(finite[:, :, :keep]), inf_counts


def _ignored_mask(truth_dev, lut: np.ndarray):
    """truth bytes that the table marks as ignored, without an int64 index volume: the ignore mark sits on few byte values"""
    import torch
    mask = torch.zeros_like(truth_dev, dtype=torch.bool)
    for value in np.flatnonzero(lut == ev.IGNORE):
        mask |= truth_dev == int(value)
    return mask


# ---- public: the figures -----------------------------------------------------------------------------------------------------------
@dataclass
class SurfaceScores:
    """Surface-distance figures per class, float64 from exact integer histograms; distances in units of ``voxel_size``."""
    truth_surface_voxels: np.ndarray            # (K,) int64
    predicted_surface_voxels: np.ndarray        # (K,) int64
    hausdorff: np.ndarray                       # the largest distance from either surface to the other
    hausdorff_95: np.ndarray                    # 95th percentile (linear interpolation) of the pooled distances
    assd: np.ndarray                            # average symmetric surface distance: the mean of the pooled distances
    mean_distance_truth_to_pred: np.ndarray
    mean_distance_pred_to_truth: np.ndarray
    surface_dice: np.ndarray                    # share of the surface voxels within the tolerance of the other surface
    truth_within_tolerance: np.ndarray          # (K,) int64
    predicted_within_tolerance: np.ndarray      # (K,) int64
    tolerance: float
    voxel_size: float
    mean_hausdorff: float                       # the means run over the classes present in truth or prediction
    mean_hausdorff_95: float
    mean_assd: float
    mean_surface_dice: float

    @property
    def classes(self) -> int:
        return int(len(self.hausdorff))


def surface_scores_from_histograms(hists, inf_counts, tolerance: float = 1.0, voxel_size: float = 1.0) -> SurfaceScores:
    """The figures of ``surface_distance_histograms``' output.  A class absent from both volumes has NaN for every figure and is left
    out of the means; a class present in only one has every distance figure ``inf`` and surface Dice 0."""
    h = np.asarray(hists).astype(np.int64)
    inf = np.asarray(inf_counts).astype(np.int64)
    if h.ndim != 3 or h.shape[1] != 2 or inf.shape != (h.shape[0], 2):
        raise ValueError(f"expected (K, 2, bins) histograms and (K, 2) counts, got {h.shape} and {inf.shape}")
    tolerance, voxel_size = float(tolerance), float(voxel_size)
    k = h.shape[0]
    dist = voxel_size * np.sqrt(np.arange(h.shape[2], dtype=np.float64))
    surf = h.sum(2) + inf                                   # (K, 2) surface voxels
    within = (h * (dist <= tolerance)).sum(2)                # (K, 2)
    figures = {name: np.full(k, np.nan) for name in ("hausdorff", "hausdorff_95", "assd", "t2p", "p2t", "dice")}
    for i in range(k):
        na, nb = int(surf[i, 0]), int(surf[i, 1])
        if na + nb == 0:
            continue
        if na == 0 or nb == 0 or inf[i].any():
            for name in ("hausdorff", "hausdorff_95", "assd", "t2p", "p2t"):
                figures[name][i] = np.inf
            figures["dice"][i] = 0.0
            continue
        pooled = h[i, 0] + h[i, 1]
        used = np.flatnonzero(pooled)
        figures["hausdorff"][i] = dist[used[-1]]
        figures["hausdorff_95"][i] = lv.percentile_from_counts(dist[used], pooled[used], 95.0)
        figures["assd"][i] = float((pooled[used] * dist[used]).sum()) / (na + nb)
        figures["t2p"][i] = float((h[i, 0, used] * dist[used]).sum()) / na
        figures["p2t"][i] = float((h[i, 1, used] * dist[used]).sum()) / nb
        figures["dice"][i] = float(within[i].sum()) / (na + nb)
    present = surf.sum(1) > 0

    def mean(x):
        return float(x[present].mean()) if present.any() else float("nan")

    return SurfaceScores(surf[:, 0].copy(), surf[:, 1].copy(), figures["hausdorff"], figures["hausdorff_95"], figures["assd"], figures["t2p"],
                         figures["p2t"], figures["dice"], within[:, 0].copy(), within[:, 1].copy(), tolerance, voxel_size,
                         mean(figures["hausdorff"]), mean(figures["hausdorff_95"]), mean(figures["assd"]), mean(figures["dice"]))


# ---- reporting ---------------------------------------------------------------------------------------------------------------------
_COLUMNS = ("truth_surface_voxels", "predicted_surface_voxels", "hausdorff", "hausdorff_95", "assd", "mean_distance_truth_to_pred",
            "mean_distance_pred_to_truth", "surface_dice", "truth_within_tolerance", "predicted_within_tolerance")
_INTEGER = {"truth_surface_voxels", "predicted_surface_voxels", "truth_within_tolerance", "predicted_within_tolerance"}


def surface_score_table(scores: SurfaceScores, label_values=None) -> str:
    """the per-class table as text, for the log"""
    values = list(range(scores.classes)) if label_values is None else [int(v) for v in label_values]
    values += [""] * (scores.classes - len(values))
    lines = [f"{'class':>5} {'value':>6} {'truth surf':>11} {'pred surf':>11} {'hausdorff':>10} {'hd95':>10} {'assd':>10} {'surf dice':>9}"]
    for i in range(scores.classes):
        lines.append(f"{i:>5} {values[i]!s:>6} {int(scores.truth_surface_voxels[i]):>11} {int(scores.predicted_surface_voxels[i]):>11} "
                     f"{scores.hausdorff[i]:>10.4f} {scores.hausdorff_95[i]:>10.4f} {scores.assd[i]:>10.4f} {scores.surface_dice[i]:>9.5f}")
    lines.append(f"mean over the classes present: hausdorff {scores.mean_hausdorff:.4f}, hd95 {scores.mean_hausdorff_95:.4f}, assd "
                 f"{scores.mean_assd:.4f}, surface dice {scores.mean_surface_dice:.5f} (tolerance {scores.tolerance:g}, voxel size {scores.voxel_size:g})")
    return "\n".join(lines)


def write_surface_scores(stem, scores: SurfaceScores, hists, inf_counts, label_values=None, grid=None) -> list[Path]:
    """``<stem>_surface_scores.csv`` (one row per class, then a ``mean`` row) and ``<stem>_surface_scores.json`` (the same figures, the
    tolerance and the voxel size, and per class the non-zero part of both histograms as squared distances and counts; NaN is
    written as null, infinity as the string "inf").  ``grid`` (``label_volume.spacing_settings``): the histograms are indexed by the
    weighted squared distance ``D``, every figure is ``unit * sqrt(D)``, and the JSON gains ``voxel_spacing``, ``weights`` and ``unit``."""
    stem = str(stem)
    k = scores.classes
    h, inf = np.asarray(hists), np.asarray(inf_counts)
    values = list(range(k)) if label_values is None else [int(v) for v in label_values]
    values += [None] * (k - len(values))
    written = [Path(stem + "_surface_scores.csv"), Path(stem + "_surface_scores.json")]
    with open(written[0], "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(("class", "label_value") + _COLUMNS)
        for i in range(k):
            w.writerow([i, "" if values[i] is None else values[i]]
                       + [int(getattr(scores, c)[i]) if c in _INTEGER else repr(float(getattr(scores, c)[i])) for c in _COLUMNS])
        w.writerow(["mean", "", "", "", repr(scores.mean_hausdorff), repr(scores.mean_hausdorff_95), repr(scores.mean_assd), "", "",
                    repr(scores.mean_surface_dice), "", ""])
    per_class = []
    for i in range(k):
        entry = dict(index=i, label_value=values[i])
        for c in _COLUMNS:
            entry[c] = int(getattr(scores, c)[i]) if c in _INTEGER else lv.json_number(getattr(scores, c)[i])
        entry["histograms"] = {}
        for d, name in enumerate(_DIRECTIONS):
            used = np.flatnonzero(h[i, d])
            entry["histograms"][name] = {"squared_distance": used.tolist(), "count": h[i, d, used].tolist(), "unreached": int(inf[i, d])}
        per_class.append(entry)
    doc = {"classes": per_class, "surface_tolerance": scores.tolerance, "voxel_size": scores.voxel_size,
           "mean_hausdorff": lv.json_number(scores.mean_hausdorff), "mean_hausdorff_95": lv.json_number(scores.mean_hausdorff_95),
           "mean_assd": lv.json_number(scores.mean_assd), "mean_surface_dice": lv.json_number(scores.mean_surface_dice)}
    if grid is not None:
        doc.update(voxel_spacing=list(grid[0]), weights=list(grid[1]), unit=grid[2])
    with open(written[1], "w") as f:
        json.dump(doc, f, indent=1)
    return written


def surface_settings(settings):
    """(enabled, tolerance, voxel size) of the optional predict-settings keys; under ``voxel_spacing`` (an error beside
    ``evaluation_voxel_size``) the tolerance is in the spacing's units and the voxel size is the grid's unit"""
    grid = lv.spacing_settings(settings, "evaluation_voxel_size")
    if grid is not None:
        return bool(getattr(settings, "evaluation_surface_distances", False)), float(getattr(settings, "evaluation_surface_tolerance", 1.0)), grid[2]
    return (bool(getattr(settings, "evaluation_surface_distances", False)), float(getattr(settings, "evaluation_surface_tolerance", 1.0)),
            float(getattr(settings, "evaluation_voxel_size", 1.0)))


def evaluate_surface_distances(pred, truth, classes: int, settings, *, label_values=None, ignore_label=None, device=None, stem=None):
    """What the evaluate command and ``evaluate_volume`` do with ``evaluation_surface_distances: true``: histograms, figures, the
    table in the log and, with ``stem``, the two files.  Returns (scores, hists, inf_counts)."""
    import logging
    _, tolerance, voxel_size = surface_settings(settings)
    grid = lv.spacing_settings(settings, "evaluation_voxel_size")
    hists, inf_counts = surface_distance_histograms(pred, truth, classes, label_values=label_values, ignore_label=ignore_label, device=device,
                                                    spacing=None if grid is None else grid[0])
    scores = surface_scores_from_histograms(hists, inf_counts, tolerance, voxel_size)
    logging.info("Surface distances against the label volume:\n" + surface_score_table(scores, label_values))
    if stem is not None:
        write_surface_scores(stem, scores, hists, inf_counts, label_values, grid)
    return scores, hists, inf_counts
