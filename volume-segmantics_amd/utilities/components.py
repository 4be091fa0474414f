"""Connected components of a label volume and the cleanup of a predicted one: drop the components of a class below a size, keep
only the largest component of a class, fill small enclosed holes.

Definitions.  Volumes are Z x Y x X (one to three dimensions), uint8 values, fewer than 2^31 voxels.  Two voxels are adjacent under
connectivity 6 (faces), 18 (faces and edges) or 26 (faces, edges and corners) - ``scipy.ndimage.generate_binary_structure(3, 1 | 2 |
3)``; an axis of length 1 has no neighbours.  A component is a maximal set of voxels of EQUAL value connected through adjacent voxels
of that value, value 0 included, so one labelling serves every class and the background.  The id of a component is the linear index
of its lowest-index voxel, its root; ``size`` is its voxel count; it ``touches`` when one of its voxels has a coordinate equal to 0 or
to extent - 1 on an axis longer than 1.

Cleanup, every decision taken from the one labelling of the INPUT.  A component of value ``c != background`` is cleared (set to
``background``) when its size is below ``min_object_size[c]``, or when ``keep_largest[c]`` and it is not the largest component of
``c`` (a tie goes to the lower root).  A background component is a hole when ``fill_holes > 0``, its size is at most ``fill_holes``,
it does not touch and its root is not voxel 0; its voxels get the final value of the voxel in front of its root (index root - 1: it
exists, and has another value, because the component does not reach the boundary) - that voxel's own value, or background when its
component is cleared, in which case the hole stays and is not counted as filled.

All routes give the same integers: the kernels of csrc/components.hip on a GPU (vs_label_components, vs_component_sizes,
vs_component_largest, vs_components_apply), ``scipy.ndimage.label`` per value on a host where scipy imports, a NumPy minimum-label
propagation otherwise (slow: small volumes)."""
from __future__ import annotations

import csv
import json
from pathlib import Path

import numpy as np

from . import label_volume as lv

TILE_Z, TILE_Y, TILE_X = 8, 8, 64      # csrc/components.hip kTZ / kTY / kTX: the tile a workgroup labels in LDS
VOXEL_LIMIT = 1 << 31                  # component ids are int32 voxel indices
_RANK = {6: 1, 18: 2, 26: 3}           # non-zero offsets a neighbour may have


# ---- arguments -------------------------------------------------------------------------------------------------------------------
def _check(shape, connectivity) -> tuple[int, int, int]:
    zyx = lv.zyx(shape)
    if int(connectivity) not in _RANK:
        raise ValueError(f"connectivity {connectivity}: it is 6, 18 or 26")
    if zyx[0] * zyx[1] * zyx[2] >= VOXEL_LIMIT:
        raise ValueError(f"a volume of shape {tuple(shape)} holds {zyx[0] * zyx[1] * zyx[2]} voxels: components need fewer than 2^31 "
                         f"(ids are int32 voxel indices)")
    return zyx


def _per_value(setting, cast, background: int, name: str) -> np.ndarray:
    """a scalar (every value but the background) or a mapping label value -> setting, as 256 entries"""
    out = np.zeros(256, dtype=np.int64)
    if isinstance(setting, dict):
        for key, value in setting.items():
            if not 0 <= int(key) <= 255:
                raise ValueError(f"{name}: label value {key} is not a uint8 value")
            out[int(key)] = cast(value)
    else:
        out[:] = cast(setting)
    out[int(background)] = 0
    if (out < 0).any():
        raise ValueError(f"{name} must not be negative")
    return out


# ---- host routes -----------------------------------------------------------------------------------------------------------------
def _offsets(connectivity: int):
    """the neighbour offsets (dz, dy, dx) that come before a voxel in index order: 3, 9 or 13"""
    rank = _RANK[connectivity]
    return [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
            if (dz, dy, dx) < (0, 0, 0) and (dz != 0) + (dy != 0) + (dx != 0) <= rank]


def _pair_slices(shape, offset):
    """slices (a, b) such that vol[a] and vol[b] are the two ends of every pair of voxels `offset` apart; None when there is none"""
    a, b = [], []
    for extent, d in zip(shape, offset):
        if abs(d) >= extent:
            return None
        a.append(slice(max(0, -d), extent - max(0, d)))
        b.append(slice(max(0, d), extent - max(0, -d)))
    return tuple(a), tuple(b)


def _roots_scipy(vol: np.ndarray, connectivity: int, ndimage) -> np.ndarray:
    n = vol.size
    structure = ndimage.generate_binary_structure(3, _RANK[connectivity])
    comp = np.empty(n, dtype=np.int32)
    index = np.arange(n, dtype=np.int32)
    for value in np.unique(vol):
        labelled, count = ndimage.label(vol == value, structure=structure, output=np.int32)
        flat = labelled.reshape(-1)
        first = np.zeros(count + 1, dtype=np.int32)
        first[flat[::-1]] = index[::-1]          # a repeated index keeps the last value assigned: the lowest voxel of each label
        member = flat != 0
        comp[member] = first[flat[member]]
    return comp.reshape(vol.shape)


def _roots_numpy(vol: np.ndarray, connectivity: int) -> np.ndarray:
    """minimum-label propagation with pointer jumping: every sweep gives a voxel the lowest id among its equal-valued neighbours, then
    follows ids to their own ids; ids only decrease and always name a voxel of the same component, so the fixed point is the root"""
    n = vol.size
    label = np.arange(n, dtype=np.int32).reshape(vol.shape)
    pairs = []
    for offset in _offsets(connectivity):
        s = _pair_slices(vol.shape, offset)
        if s is not None:
            same = vol[s[0]] == vol[s[1]]
            if same.any():
                pairs.append((s[0], s[1], same))
    while True:
        new = label.copy()
        for a, b, same in pairs:
            low = np.minimum(new[a], new[b])
            np.minimum(new[a], low, out=new[a], where=same)          # the two views overlap: take minima, never overwrite a lower id
            np.minimum(new[b], low, out=new[b], where=same)
        flat = new.reshape(-1)
        while True:
            jumped = flat[flat]
            if np.array_equal(jumped, flat):
                break
            flat = jumped
        new = flat.reshape(vol.shape)
        if np.array_equal(new, label):
            return label
        label = new


def _roots_host(vol: np.ndarray, connectivity: int, use_scipy=None) -> np.ndarray:
    ndimage = None
    if use_scipy is not False:
        try:
            from scipy import ndimage
        except ImportError:
            if use_scipy:
                raise
    return _roots_scipy(vol, connectivity, ndimage) if ndimage is not None else _roots_numpy(vol, connectivity)


def _table_host(vol: np.ndarray, comp: np.ndarray):
    """per component, roots ascending: root, size, value, touches, and the value and root of the voxel in front of the root"""
    flat_v, flat_c = vol.reshape(-1), comp.reshape(-1)
    size = np.bincount(flat_c, minlength=flat_c.size)
    roots = np.flatnonzero(size)
    touch = np.zeros(flat_c.size, dtype=bool)
    touch[flat_c[lv.touch_mask(vol.shape).reshape(-1)]] = True
    front = np.maximum(roots - 1, 0)
    return dict(roots=roots.astype(np.int64), sizes=size[roots].astype(np.int64), values=flat_v[roots].astype(np.int64), touches=touch[roots],
                front_values=flat_v[front].astype(np.int64), front_roots=flat_c[front].astype(np.int64))


# ---- device routes ---------------------------------------------------------------------------------------------------------------
def _device_bytes(zyx, on_device: bool) -> int:
    """the upload unless the volume is there, the roots, sizes, touches, the cleaned copy and the workspace"""
    from .. import _lib
    n = zyx[0] * zyx[1] * zyx[2]
    return (0 if on_device else n) + 4 * n + 4 * n + n + n + int(_lib.lib.vs_components_workspace_bytes(*zyx))


def label_device(labels_dev, zyx, connectivity):
    """vs_label_components on flat aligned device bytes: the int32 root of every voxel, on the device"""
    import torch
    from .. import _lib
    n = labels_dev.numel()
    comp = torch.empty(n, dtype=torch.int32, device=labels_dev.device)
    work = torch.empty(int(_lib.lib.vs_components_workspace_bytes(*zyx)), dtype=torch.uint8, device=labels_dev.device)
    with torch.cuda.device(labels_dev.device):
        _lib.check(_lib.lib.vs_label_components(_lib.ptr(labels_dev), *zyx, int(connectivity), _lib.ptr(comp), _lib.ptr(work), work.numel(),
                                                _lib.stream_ptr()))
    return comp


def sizes_device(comp, zyx):
    """vs_component_sizes: (int32 size, uint8 touches) at every root, 0 elsewhere, on the device"""
    import torch
    from .. import _lib
    size = torch.empty(comp.numel(), dtype=torch.int32, device=comp.device)
    touches = torch.empty(comp.numel(), dtype=torch.uint8, device=comp.device)
    with torch.cuda.device(comp.device):
        _lib.check(_lib.lib.vs_component_sizes(_lib.ptr(comp), *zyx, _lib.ptr(size), _lib.ptr(touches), _lib.stream_ptr()))
    return size, touches


def _table_device(labels_dev, comp, size, touches):
    import torch
    roots = torch.nonzero(size).reshape(-1)              # the compaction: ascending
    front = torch.clamp(roots - 1, min=0)
    host = lambda t: t.cpu().numpy().astype(np.int64)    # noqa: E731
    return dict(roots=host(roots), sizes=host(size[roots]), values=host(labels_dev[roots]), touches=touches[roots].cpu().numpy() != 0,
                front_values=host(labels_dev[front]), front_roots=host(comp[front]))


def _largest_device(labels_dev, size):
    """256 roots: the largest component of each value (vs_component_largest), -1 where the value does not occur"""
    import torch
    from .. import _lib
    keys = torch.empty(256, dtype=torch.int64, device=size.device)
    with torch.cuda.device(size.device):
        _lib.check(_lib.lib.vs_component_largest(_lib.ptr(labels_dev), _lib.ptr(size), size.numel(), _lib.ptr(keys), _lib.stream_ptr()))
    k = keys.cpu().numpy()
    return np.where(k != 0, 0x7FFFFFFF - (k & 0xFFFFFFFF), -1).astype(np.int64)


def prepare(vol, connectivity, device):
    """``label_volume.prepare`` after the checks of a labelling, with the device memory one takes: (shape, zyx, device or None, volume)"""
    _check(tuple(vol.shape), connectivity)
    return lv.prepare(vol, device, _device_bytes, "components")


# ---- public: the pieces ------------------------------------------------------------------------------------------------------------
def label_components(vol, connectivity: int = 6, device=None) -> np.ndarray:
    """int32 array of ``vol.shape``: for every voxel the root of its component (the linear index of the component's lowest voxel)."""
    shape, zyx, device, v = prepare(vol, connectivity, device)
    if device is None:
        return _roots_host(v, int(connectivity)).reshape(shape)
    return label_device(v, zyx, connectivity).cpu().numpy().reshape(shape)


def _largest_of(table) -> np.ndarray:
    """256 roots: per value the largest component, the lower root on a tie; -1 where the value does not occur"""
    best = np.full(256, -1, dtype=np.int64)
    order = np.lexsort((table["roots"], -table["sizes"], table["values"]))       # by value, then size descending, then root ascending
    values = table["values"][order]
    first = np.ones(len(values), dtype=bool)
    first[1:] = values[1:] != values[:-1]
    best[values[first]] = table["roots"][order][first]
    return best


def component_table(vol, connectivity: int = 6, device=None) -> dict:
    """``{label value: {"components": count, "sizes": [voxel counts, descending]}}`` for every value that occurs."""
    _, zyx, device, v = prepare(vol, connectivity, device)
    if device is None:
        table = _table_host(v, _roots_host(v, int(connectivity)))
    else:
        comp = label_device(v, zyx, connectivity)
        table = _table_device(v, comp, *sizes_device(comp, zyx))
    out = {}
    for value in np.unique(table["values"]):
        sizes = np.sort(table["sizes"][table["values"] == value])[::-1]
        out[int(value)] = {"components": int(len(sizes)), "sizes": sizes.tolist()}
    return out


def _decide(table, min_size, keep_root, hole_max: int, background: int):
    """per component: whether it is cleared, and the value a hole is filled with (-1: not a hole that changes)"""
    roots, sizes, values = table["roots"], table["sizes"], table["values"]
    object_ = values != background
    cleared = object_ & ((sizes < min_size[values]) | ((keep_root[values] >= 0) & (roots != keep_root[values])))
    fill = np.full(len(roots), -1, dtype=np.int64)
    if hole_max > 0:
        hole = ~object_ & (sizes <= hole_max) & ~table["touches"] & (roots > 0)
        front_cleared = np.zeros(len(roots), dtype=bool)
        if hole.any():
            position = np.searchsorted(roots, table["front_roots"][hole])
            front_cleared[hole] = cleared[position]
        filled = hole & ~front_cleared & (table["front_values"] != background)
        fill[filled] = table["front_values"][filled]
    return cleared, fill


def _report(table, cleared, fill, settings: dict) -> dict:
    values, sizes = table["values"], table["sizes"]
    per_value = {}
    for value in np.unique(values):
        mine = values == value
        gone = mine & cleared
        per_value[str(int(value))] = {
            "components": int(mine.sum()), "voxels": int(sizes[mine].sum()),
            "components_cleared": int(gone.sum()), "voxels_cleared": int(sizes[gone].sum()),
            "components_kept": int((mine & ~cleared).sum()), "voxels_kept": int(sizes[mine & ~cleared].sum())}
    return dict(settings, values=per_value, holes_filled=int((fill >= 0).sum()), voxels_filled=int(sizes[fill >= 0].sum()))


def _clean_host(vol: np.ndarray, comp: np.ndarray, min_size, keep, hole_max: int, background: int, settings: dict):
    """the host route of ``clean_label_volume`` from the roots ``comp`` of ``vol``"""
    table = _table_host(vol, comp)
    keep_root = np.where(keep, _largest_of(table), -1)
    cleared, fill = _decide(table, min_size, keep_root, hole_max, background)
    final = np.zeros(vol.size, dtype=np.uint8)
    final[table["roots"]] = np.where(cleared, background, np.where(fill >= 0, fill, table["values"]))
    return final[comp.reshape(-1)].reshape(vol.shape), _report(table, cleared, fill, settings)


def clean_label_volume(vol, min_object_size=0, keep_largest=False, fill_holes: int = 0, connectivity: int = 6, background: int = 0, device=None):
    """(cleaned uint8 array of ``vol.shape``, report).  ``min_object_size`` and ``keep_largest`` are each a scalar - it then holds for
    every value but the background - or a mapping from label value to setting.  The report holds the settings, per label value
    (``report["values"][str(value)]``) the components and voxels before, cleared and kept, and ``holes_filled`` / ``voxels_filled``
    (kept counts are those before any hole is filled)."""
    background, fill_holes, connectivity = int(background), int(fill_holes), int(connectivity)
    if not 0 <= background <= 255:
        raise ValueError(f"background {background} is not a uint8 value")
    if fill_holes < 0:
        raise ValueError("fill_holes must not be negative")
    min_size = _per_value(min_object_size, int, background, "min_object_size")
    keep = _per_value(keep_largest, lambda x: int(bool(x)), background, "keep_largest") != 0
    shape, zyx, device, v = prepare(vol, connectivity, device)
    settings = dict(connectivity=connectivity, background=background, fill_holes=fill_holes,
                    min_object_size={str(c): int(min_size[c]) for c in np.flatnonzero(min_size)},
                    keep_largest=[int(c) for c in np.flatnonzero(keep)])
    hole_max = min(fill_holes, VOXEL_LIMIT - 1)
    if device is None:
        cleaned, report = _clean_host(v, _roots_host(v, connectivity), min_size, keep, hole_max, background, settings)
        return cleaned.reshape(shape), report

    import torch
    from .. import _lib
    comp = label_device(v, zyx, connectivity)
    size, touches = sizes_device(comp, zyx)
    keep_root = np.where(keep, _largest_device(v, size), -1)
    out = torch.empty_like(v)
    counts = torch.empty(4, dtype=torch.int64, device=device)
    min_dev = torch.from_numpy(np.minimum(min_size, VOXEL_LIMIT - 1).astype(np.int32)).to(device)
    keep_dev = torch.from_numpy(keep_root.astype(np.int32)).to(device)
    with torch.cuda.device(device):
        _lib.check(_lib.lib.vs_components_apply(_lib.ptr(v), _lib.ptr(comp), _lib.ptr(size), _lib.ptr(touches), _lib.ptr(min_dev), _lib.ptr(keep_dev),
                                                background, hole_max, v.numel(), _lib.ptr(out), _lib.ptr(counts), _lib.stream_ptr()))
    table = _table_device(v, comp, size, touches)
    cleared, fill = _decide(table, min_size, keep_root, hole_max, background)
    report = _report(table, cleared, fill, settings)
    want = [int(cleared.sum()), int(table["sizes"][cleared].sum()), report["holes_filled"], report["voxels_filled"]]
    if counts.cpu().tolist() != want:
        raise RuntimeError(f"the cleanup kernel counted {counts.cpu().tolist()} (components and voxels cleared, holes and voxels filled), "
                           f"the component table gives {want}")
    return out.cpu().numpy().reshape(shape), report


# ---- settings and reporting ------------------------------------------------------------------------------------------------------
def postprocess_settings(settings) -> dict:
    """the optional predict-settings keys ``postprocess_min_object_size``, ``postprocess_keep_largest``, ``postprocess_fill_holes`` and
    ``postprocess_connectivity`` as ``clean_label_volume`` arguments, plus ``active``: whether any of the first three asks for work"""
    def is_set(x):
        return any(bool(v) for v in x.values()) if isinstance(x, dict) else bool(x)

    min_object_size = getattr(settings, "postprocess_min_object_size", 0) or 0
    keep_largest = getattr(settings, "postprocess_keep_largest", False) or False
    fill_holes = int(getattr(settings, "postprocess_fill_holes", 0) or 0)
    connectivity = int(getattr(settings, "postprocess_connectivity", 6) or 6)
    if connectivity not in _RANK:
        raise ValueError(f"postprocess_connectivity {connectivity}: it is 6, 18 or 26")
    return dict(active=is_set(min_object_size) or is_set(keep_largest) or fill_holes > 0, min_object_size=min_object_size,
                keep_largest=keep_largest, fill_holes=fill_holes, connectivity=connectivity)


def postprocess_label_volume(vol, settings, device=None):
    """``clean_label_volume`` with the settings keys; (cleaned, report)"""
    p = postprocess_settings(settings)
    return clean_label_volume(vol, p["min_object_size"], p["keep_largest"], p["fill_holes"], p["connectivity"], device=device)


_COLUMNS = ("components", "voxels", "components_cleared", "voxels_cleared", "components_kept", "voxels_kept")


def component_report_table(report: dict) -> str:
    """the per-value table as text, for the log"""
    lines = [f"{'value':>5} {'components':>10} {'voxels':>12} {'cleared':>10} {'vox cleared':>12} {'kept':>10} {'vox kept':>12}"]
    for value, row in report["values"].items():
        lines.append(f"{value:>5} " + " ".join(f"{row[c]:>{w}}" for c, w in zip(_COLUMNS, (10, 12, 10, 12, 10, 12))))
    lines.append(f"holes filled: {report['holes_filled']} ({report['voxels_filled']} voxels); connectivity {report['connectivity']}")
    return "\n".join(lines)


def write_component_report(stem, report: dict) -> list[Path]:
    """``<stem>_components.json`` (the report) and ``<stem>_components.csv`` (one row per label value, then a ``holes`` row)."""
    stem = str(stem)
    written = [Path(stem + "_components.json"), Path(stem + "_components.csv")]
    with open(written[0], "w") as f:
        json.dump(report, f, indent=1)
    with open(written[1], "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(("label_value",) + _COLUMNS)
        for value, row in report["values"].items():
            w.writerow([value] + [row[c] for c in _COLUMNS])
        w.writerow(["holes", report["holes_filled"], report["voxels_filled"], "", "", "", ""])
    return written
