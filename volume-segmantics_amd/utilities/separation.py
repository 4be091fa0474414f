"""Touching objects apart: a watershed on the distance map of a label value, so that ``measure_objects`` lists grains, particles,
pores or cells one by one where a connected component would lump every object that touches another into one row.

Definitions (exact integers; every route gives the same bits).  Volumes, neighbourhoods (6 / 18 / 26), "an axis of length 1 has no
neighbours" and roots are those of ``utilities/components.py``; the connectivity ``N`` serves the components, the ascent and the
adjacency of basins alike.  For a label value ``c`` with voxels ``M``:

1. ``R(v)`` is the squared distance from ``v`` to the nearest in-volume voxel whose value is not ``c`` (``vs_edt_squared`` with the seeds
   ``labels != c`` - the convention of ``utilities/thickness.py``: outside the volume is not background) and 0 off ``M``.  A value
   beside which the volume holds no other value is not separated: its components stay, and the report says so.
2. Every voxel of ``M`` has the key ``K(v) = (R(v) << 32) | (0xFFFFFFFF - v)``: all keys differ, the higher ``R`` wins, then the lower
   index.  ``parent(v)`` holds the largest key among ``v`` and its ``N``-neighbours; a voxel that is its own parent is a peak; keys strictly
   increase along ``v -> parent(v) -> ...``, so every chain ends at a peak, and the basin of a peak is the set of voxels whose chain
   ends there.
3. The pair table has one row per unordered pair of basins ``A < B`` (peak indices) that hold ``N``-adjacent voxels ``u`` in ``A``, ``v`` in
   ``B``: the saddle ``S(A, B)`` = the largest ``min(R(u), R(v))`` over such pairs, and ``faces_z / _y / _x`` = the face-adjacent ones
   across each axis.
4. The merge (``merge_basins``: host code, ONE implementation for both routes) sorts the rows by (``S`` descending, ``A``, ``B``) and runs
   union-find over the peaks with ``H(set)`` = the largest ``R`` of its peaks: a row whose ends lie in different sets ``a``, ``b`` unites
   them when ``sqrt(float64(min(H(a), H(b)))) - sqrt(float64(S)) < depth``.  ``depth`` is in unit voxels: 0 keeps the raw basins, infinity
   gives back the components.
5. ``objects[v]`` is the lowest voxel index of ``v``'s merged set; voxels of values that were not separated keep the root of their
   component.  ``objects`` refines the component labelling and is taken by everything that takes a ``comp`` by id.
6. The contact of two objects of one value: ``neck`` = the largest ``S`` over the table rows between them, the faces summed over them.

Routes: ``vs_separate_parents`` / ``_basins`` / ``_pair_count`` / ``_pairs`` / ``_relabel`` (csrc/separate.hip) behind ``vs_edt_squared`` and
``vs_label_components`` on a GPU; NumPy behind ``surface_distance.squared_distance_transform`` on a host, for small volumes and for
parity.  A value whose pair table has more than ``max_pairs`` rows is refused: that is debris, not objects.

Anisotropic voxels (``voxel_spacing: [sz, sy, sx]``, ``spacing=``): ``R``, the peaks and the saddles are the weighted integers ``D = qz dz^2 +
qy dy^2 + qx dx^2`` of ``label_volume.voxel_grid`` (``vs_edt_squared_scaled``; the kernels of csrc/separate.hip consume ``R`` as it comes).
``depth`` stays in voxels of the finest axis: the merge compares ``(sqrt(H) - sqrt(S)) / w_min``, ``w_min`` the smallest weight, so an
isotropic spacing gives the same objects bit for bit.  ``neck_radius`` is then ``unit * sqrt(neck_squared)``.

Not here: markers from the user, smoothing of the distance map, a watershed on image
intensity, separated objects in the scores of ``evaluate``, in the meshes or in the thickness report."""
from __future__ import annotations

import csv
import json
import math
from pathlib import Path

import numpy as np

from . import components as co
from . import label_volume as lv
from . import surface_distance as sd

DEFAULT_DEPTH = 1.0
DEFAULT_MAX_PAIRS = 5_000_000
CONTACT_COLUMNS = ("id_a", "id_b", "value", "faces_z", "faces_y", "faces_x", "contact_area", "neck_squared", "neck_radius")


# ---- arguments -------------------------------------------------------------------------------------------------------------------
def _check_depth(depth) -> float:
    depth = float(depth)
    if math.isnan(depth) or depth < 0:
        raise ValueError(f"the separation depth {depth} must be a number of voxels of at least 0 (inf gives back the components)")
    return depth


def _check_values(values, present) -> list[int]:
    if values is None:
        return [int(c) for c in present if c != 0]
    out = sorted({int(c) for c in (values if isinstance(values, (list, tuple, np.ndarray)) else [values])})
    for c in out:
        if not 0 <= c <= 255:
            raise ValueError(f"value {c} is not a uint8 value")
    return out


def _check_pairs(rows: int, max_pairs, value: int) -> None:
    if max_pairs is not None and rows > max_pairs:
        raise ValueError(f"the pair table of value {value} has {rows} rows, more than measure_separate_max_pairs = {int(max_pairs)}: separation is "
                         f"asked of volumes with objects, not of debris - raise the key, or leave the value out of measure_separate_values")


def table_slots(count: int, basins: int) -> int:
    """the size of the pair table: a power of two at or above twice the smaller of the adjacent voxel pairs and B (B - 1) / 2"""
    bound = min(int(count), basins * (basins - 1) // 2)
    return 1 << max(2 * bound - 1, 1).bit_length()


# ---- host route: the stages ------------------------------------------------------------------------------------------------------
_RANK = {6: 1, 18: 2, 26: 3}           # non-zero offsets a neighbour may have


def _forward_offsets(connectivity: int):
    """the neighbour offsets (dz, dy, dx) that come before a voxel in index order: 3, 9 or 13 - every adjacent pair once, at its later voxel"""
    rank = _RANK[int(connectivity)]
    return [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
            if (dz, dy, dx) < (0, 0, 0) and (dz != 0) + (dy != 0) + (dx != 0) <= rank]


def _all_offsets(connectivity: int):
    before = _forward_offsets(connectivity)
    return before + [(-dz, -dy, -dx) for dz, dy, dx in before]


def _pair_slices(shape, offset):
    """slices (a, b) such that vol[a] and vol[b] are the two ends of every pair of voxels `offset` apart; None when there is none"""
    a, b = [], []
    for extent, d in zip(shape, offset):
        if abs(d) >= extent:
            return None
        a.append(slice(max(0, -d), extent - max(0, d)))
        b.append(slice(max(0, d), extent - max(0, -d)))
    return tuple(a), tuple(b)


def ascent_parents(r: np.ndarray, connectivity: int = 6) -> np.ndarray:
    """int32 array of ``r.shape`` ((Z, Y, X) uint32): the parent of every voxel with ``r > 0``, -1 elsewhere"""
    r = np.asarray(r)
    n = r.size
    index = np.arange(n, dtype=np.uint64).reshape(r.shape)
    key = np.where(r > 0, (r.astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - index), np.uint64(0))      # off the value: below every key
    best = key.copy()
    for offset in _all_offsets(int(connectivity)):
        s = _pair_slices(r.shape, offset)
        if s is not None:
            np.maximum(best[s[1]], key[s[0]], out=best[s[1]])
    parent = (np.uint64(0xFFFFFFFF) - (best & np.uint64(0xFFFFFFFF))).astype(np.int64)
    return np.where(r > 0, parent, -1).astype(np.int32)


def basins(parent: np.ndarray) -> np.ndarray:
    """int32 array of ``parent.shape``: the peak at which the chain of every voxel ends (pointer jumping to the fixed point), -1 stays"""
    flat = np.asarray(parent).reshape(-1).astype(np.int64)
    member = np.flatnonzero(flat >= 0)
    at = flat[member]
    while True:
        jumped = flat[at]
        if np.array_equal(jumped, at):
            break
        flat[member] = at = jumped
    return flat.astype(np.int32).reshape(np.asarray(parent).shape)


def basin_pairs(r: np.ndarray, basin: np.ndarray, connectivity: int = 6) -> dict:
    """The pair table sorted by key, as int64 arrays: ``a``, ``b``, ``saddle`` (rows,), ``faces`` (rows, 3), and ``count``: the adjacent voxel
    pairs in different basins (what ``vs_separate_pair_count`` gives)."""
    r, basin = np.asarray(r), np.asarray(basin)
    keys, saddles, axes = [], [], []
    for offset in _forward_offsets(connectivity):
        s = _pair_slices(r.shape, offset)
        if s is None:
            continue
        ba, bb = basin[s[0]].astype(np.int64), basin[s[1]].astype(np.int64)
        differ = (ba >= 0) & (bb >= 0) & (ba != bb)
        if not differ.any():
            continue
        ba, bb = ba[differ], bb[differ]
        keys.append((np.minimum(ba, bb) << 32) | np.maximum(ba, bb))
        saddles.append(np.minimum(r[s[0]][differ], r[s[1]][differ]).astype(np.int64))
        nonzero = [i for i, d in enumerate(offset) if d != 0]
        axes.append(np.full(len(ba), nonzero[0] if len(nonzero) == 1 else -1, dtype=np.int64))
    if not keys:
        empty = np.zeros(0, dtype=np.int64)
        return dict(a=empty, b=empty, saddle=empty, faces=np.zeros((0, 3), dtype=np.int64), count=0)
    key, saddle, axis = np.concatenate(keys), np.concatenate(saddles), np.concatenate(axes)
    order = np.argsort(key, kind="stable")
    key, saddle, axis = key[order], saddle[order], axis[order]
    unique, starts = np.unique(key, return_index=True)
    faces = np.stack([np.add.reduceat((axis == k).astype(np.int64), starts) for k in range(3)], axis=1)
    return dict(a=unique >> 32, b=unique & 0xFFFFFFFF, saddle=np.maximum.reduceat(saddle, starts), faces=faces, count=int(len(key)))


# ---- the merge: shared by both routes ----------------------------------------------------------------------------------------------
def merge_basins(peaks, peak_r, a, b, saddle, depth: float, finest: int = 1):
    """(int64 array aligned with ``peaks``: the representative - the lowest peak - of every peak's merged set, the merges made).
    ``peaks`` ascending voxel indices, ``peak_r`` their R, (``a``, ``b``, ``saddle``) the rows of the pair table.  ``finest``: the smallest weight
    of a weighted grid, which turns the weighted ``sqrt(H) - sqrt(S)`` into voxels of the finest axis."""
    finest = float(finest)
    depth = _check_depth(depth)
    peaks = np.asarray(peaks, dtype=np.int64)
    position = {int(p): i for i, p in enumerate(peaks.tolist())}
    link = list(range(len(peaks)))
    height = [int(h) for h in np.asarray(peak_r).tolist()]

    def find(i):
        root = i
        while link[root] != root:
            root = link[root]
        while link[i] != root:
            link[i], i = root, link[i]
        return root

    a, b, saddle = (np.asarray(t, dtype=np.int64) for t in (a, b, saddle))
    merges = 0
    for row in np.lexsort((b, a, -saddle)).tolist():                   # saddle descending, then A, then B
        fa, fb = find(position[int(a[row])]), find(position[int(b[row])])
        if fa != fb and (math.sqrt(float(min(height[fa], height[fb]))) - math.sqrt(float(saddle[row]))) / finest < depth:
            lo, hi = min(fa, fb), max(fa, fb)                            # peaks ascend with their position: the lowest peak stays the root
            link[hi] = lo
            height[lo] = max(height[fa], height[fb])
            merges += 1
    return peaks[[find(i) for i in range(len(peaks))]] if len(peaks) else peaks, merges


def _contacts_of(value: int, table: dict, object_of_a, object_of_b) -> dict:
    """the rows of the pair table between different final objects, grouped by the pair of objects"""
    oa, ob = np.asarray(object_of_a, dtype=np.int64), np.asarray(object_of_b, dtype=np.int64)
    apart = oa != ob
    lo, hi = np.minimum(oa, ob)[apart], np.maximum(oa, ob)[apart]
    if not len(lo):
        return _no_contacts()
    key = (lo << 32) | hi
    order = np.argsort(key, kind="stable")
    unique, starts = np.unique(key[order], return_index=True)
    return dict(root_a=unique >> 32, root_b=unique & 0xFFFFFFFF, value=np.full(len(unique), value, dtype=np.int64),
                faces=np.add.reduceat(table["faces"][apart][order], starts, axis=0), neck_squared=np.maximum.reduceat(table["saddle"][apart][order], starts))


def _no_contacts() -> dict:
    empty = np.zeros(0, dtype=np.int64)
    return dict(root_a=empty, root_b=empty, value=empty, faces=np.zeros((0, 3), dtype=np.int64), neck_squared=empty)


def _join_contacts(parts) -> dict:
    parts = list(parts) or [_no_contacts()]
    return {name: np.concatenate([p[name] for p in parts]) for name in parts[0]}


def _not_separated(components: int, why: str) -> dict:
    return dict(components=components, separated=False, why=why, basins=0, pair_rows=0, adjacent_pairs=0, merges=0, objects=components)


# ---- host route ------------------------------------------------------------------------------------------------------------------
def _value_host(v: np.ndarray, value: int, connectivity: int, depth: float, max_pairs, objects: np.ndarray, components: int, weights=lv.UNIT_WEIGHTS):
    member = v == value
    if not member.any():
        return _not_separated(0, "the volume does not hold the value"), _no_contacts()
    if member.all():
        return _not_separated(components, "the volume holds no other value: there is no distance map"), _no_contacts()
    unit = tuple(weights) == lv.UNIT_WEIGHTS
    r = sd.squared_distance_transform(~member, device="cpu").reshape(v.shape) if unit else sd.edt_host(~member, weights)
    r = np.where(member, r, 0).astype(np.uint32)
    basin = basins(ascent_parents(r, connectivity)).reshape(-1)
    table = basin_pairs(r, basin.reshape(v.shape), connectivity)
    _check_pairs(len(table["a"]), max_pairs, value)
    peaks = np.flatnonzero(basin == np.arange(basin.size))
    rep, merges = merge_basins(peaks, r.reshape(-1)[peaks], table["a"], table["b"], table["saddle"], depth, min(weights))
    set_of_peak = np.full(basin.size, -1, dtype=np.int64)
    set_of_peak[peaks] = rep
    inside = np.flatnonzero(basin >= 0)
    rep_of_voxel = set_of_peak[basin[inside]]
    lowest = np.full(basin.size, basin.size, dtype=np.int64)
    np.minimum.at(lowest, rep_of_voxel, inside)
    objects[inside] = lowest[rep_of_voxel]
    contacts = _contacts_of(value, table, objects[table["a"]], objects[table["b"]])
    report = dict(components=components, separated=True, why=None, basins=int(len(peaks)), pair_rows=int(len(table["a"])),
                  adjacent_pairs=int(table["count"]), merges=int(merges), objects=int(len(peaks) - merges))
    return report, contacts


def _components_per_value(flat_v, flat_comp) -> np.ndarray:
    roots = np.flatnonzero(flat_comp == np.arange(flat_comp.size))
    return np.bincount(flat_v[roots], minlength=256)


def _separate_host(v: np.ndarray, values, connectivity: int, depth: float, max_pairs, weights=lv.UNIT_WEIGHTS):
    comp = co.label_components(v, connectivity, device="cpu")
    objects = comp.reshape(-1).astype(np.int32).copy()
    per_value = _components_per_value(v.reshape(-1), objects)
    values = _check_values(values, np.unique(v))
    report, contacts = {}, []
    for value in values:
        report[str(value)], c = _value_host(v, value, connectivity, depth, max_pairs, objects, int(per_value[value]), weights)
        contacts.append(c)
    return objects, report, _join_contacts(contacts)


# ---- device route ----------------------------------------------------------------------------------------------------------------
def parents_device(r, zyx, connectivity: int):
    """vs_separate_parents on n int32 (uint32 bits) of device memory: the int32 parents, on the device"""
    import torch
    from .. import _lib
    parent = torch.empty(r.numel(), dtype=torch.int32, device=r.device)
    with torch.cuda.device(r.device):
        _lib.check(_lib.lib.vs_separate_parents(_lib.ptr(r), *zyx, int(connectivity), _lib.ptr(parent), _lib.stream_ptr()))
    return parent


def basins_device(parent, zyx):
    """vs_separate_basins, in place"""
    import torch
    from .. import _lib
    with torch.cuda.device(parent.device):
        _lib.check(_lib.lib.vs_separate_basins(_lib.ptr(parent), *zyx, _lib.stream_ptr()))
    return parent


def pair_count_device(basin, zyx, connectivity: int) -> int:
    import torch
    from .. import _lib
    count = torch.empty(1, dtype=torch.int64, device=basin.device)
    with torch.cuda.device(basin.device):
        _lib.check(_lib.lib.vs_separate_pair_count(_lib.ptr(basin), *zyx, int(connectivity), _lib.ptr(count), _lib.stream_ptr()))
    return int(count.item())


def pairs_device(r, basin, zyx, connectivity: int, slots: int) -> dict:
    """vs_separate_pairs into a table of ``slots`` slots, then the occupied slots sorted by key - the form of ``basin_pairs`` (without
    ``count``).  A table that is too small raises RuntimeError with the library's message."""
    import torch
    from .. import _lib
    device = r.device
    keys = torch.empty(slots, dtype=torch.int64, device=device)
    saddle = torch.empty(slots, dtype=torch.int32, device=device)
    faces = torch.empty((slots, 3), dtype=torch.int32, device=device)
    used = torch.empty(2, dtype=torch.int64, device=device)
    with torch.cuda.device(device):
        _lib.check(_lib.lib.vs_separate_pairs(_lib.ptr(r), _lib.ptr(basin), *zyx, int(connectivity), _lib.ptr(keys), _lib.ptr(saddle), _lib.ptr(faces),
                                              slots, _lib.ptr(used), _lib.stream_ptr()))
    taken = torch.nonzero(keys != -1).reshape(-1)                      # the free mark reads -1 as int64
    if int(used[0]) != taken.numel():
        raise RuntimeError(f"the pair table counts {int(used[0])} claimed slots but holds {taken.numel()} keys")
    key, order = torch.sort(keys[taken])                               # peaks are below 2^31: the keys are positive
    taken = taken[order]
    host = lambda t: t.cpu().numpy().astype(np.int64)                 # noqa: E731
    key = host(key)
    return dict(a=key >> 32, b=key & 0xFFFFFFFF, saddle=host(saddle[taken]) & 0xFFFFFFFF, faces=host(faces[taken]).reshape(-1, 3))


def relabel_device(basin, set_of_peak, zyx, objects):
    """vs_separate_relabel: ``objects`` (n int32 on the device) receives the lowest voxel of every merged set at the voxels of ``basin``"""
    import torch
    from .. import _lib
    work = torch.empty(int(_lib.lib.vs_separate_workspace_bytes(*zyx)), dtype=torch.uint8, device=basin.device)
    with torch.cuda.device(basin.device):
        _lib.check(_lib.lib.vs_separate_relabel(_lib.ptr(basin), _lib.ptr(set_of_peak), *zyx, _lib.ptr(objects), _lib.ptr(work), work.numel(),
                                                _lib.stream_ptr()))
    return objects


def _value_device(v, zyx, value: int, connectivity: int, depth: float, max_pairs, objects, components: int, weights=lv.UNIT_WEIGHTS):
    import torch
    from .. import _lib
    device, n = v.device, v.numel()
    member = v == value
    voxels = int(member.sum())
    if voxels == 0:
        return _not_separated(0, "the volume does not hold the value"), _no_contacts()
    if voxels == n:
        return _not_separated(components, "the volume holds no other value: there is no distance map"), _no_contacts()
    edt_bytes = int(_lib.lib.vs_edt_workspace_bytes(*zyx))
    lv.require_memory(device, n + 4 * n + edt_bytes + 4 * n + 4 * n + 4 * n, f"the distance map, the basins and the relabelling of value {value} of a {tuple(zyx)} volume")
    seeds = (~member).to(torch.uint8)
    r = torch.empty(n, dtype=torch.int32, device=device)
    sd.edt_device(seeds, zyx, r, torch.empty(edt_bytes, dtype=torch.uint8, device=device), weights)
    del seeds                                                          # r is 0 at the seeds: off the value
    basin = basins_device(parents_device(r, zyx, connectivity), zyx)
    peaks = torch.nonzero(basin == torch.arange(n, dtype=torch.int32, device=device)).reshape(-1)      # ascending
    count = pair_count_device(basin, zyx, connectivity)
    slots = table_slots(count, int(peaks.numel()))
    lv.require_memory(device, 24 * slots + 64, f"the pair table of value {value}: {slots} slots for {count} adjacent pairs of voxels in different basins")
    table = pairs_device(r, basin, zyx, connectivity, slots)
    _check_pairs(len(table["a"]), max_pairs, value)
    peaks_host = peaks.cpu().numpy().astype(np.int64)
    peak_r = (r[peaks].cpu().numpy().astype(np.int64)) & 0xFFFFFFFF
    rep, merges = merge_basins(peaks_host, peak_r, table["a"], table["b"], table["saddle"], depth, min(weights))
    set_of_peak = torch.full((n,), -1, dtype=torch.int32, device=device)
    set_of_peak[peaks] = torch.from_numpy(rep.astype(np.int32)).to(device)
    relabel_device(basin, set_of_peak, zyx, objects)
    both = torch.from_numpy(np.concatenate([table["a"], table["b"]])).to(device)
    of = objects[both].cpu().numpy().astype(np.int64)
    contacts = _contacts_of(value, table, of[:len(table["a"])], of[len(table["a"]):])
    report = dict(components=components, separated=True, why=None, basins=int(len(peaks_host)), pair_rows=int(len(table["a"])),
                  adjacent_pairs=int(count), merges=int(merges), objects=int(len(peaks_host) - merges))
    return report, contacts


def separate_device(v, zyx, values, connectivity: int, depth: float, max_pairs, weights=lv.UNIT_WEIGHTS):
    """(objects: n int32 on the device, report, contacts) from flat aligned uint8 device memory"""
    import torch
    n = v.numel()
    objects = co.label_device(v, zyx, connectivity)
    roots = torch.nonzero(objects == torch.arange(n, dtype=torch.int32, device=v.device)).reshape(-1)
    per_value = torch.bincount(v[roots].to(torch.int64), minlength=256).cpu().numpy()
    values = _check_values(values, torch.unique(v).cpu().numpy())
    report, contacts = {}, []
    for value in values:
        report[str(value)], c = _value_device(v, zyx, value, connectivity, depth, max_pairs, objects, int(per_value[value]), weights)
        contacts.append(c)
    return objects, report, _join_contacts(contacts)


# ---- public ------------------------------------------------------------------------------------------------------------------------
def separate_prepared(v, zyx, device, values, connectivity: int, depth: float, max_pairs, weights=lv.UNIT_WEIGHTS):
    """``separate_objects`` on what ``components.prepare`` returned: objects flat, on the host or on the device; ``weights``: the integer
    weights of the axes in the distance map"""
    depth = _check_depth(depth)
    weights = lv.check_weights(weights, zyx)
    if device is None:
        return _separate_host(v, values, int(connectivity), depth, max_pairs, weights)
    return separate_device(v, zyx, values, int(connectivity), depth, max_pairs, weights)


def separate_objects(vol, values=None, connectivity: int = 6, depth: float = DEFAULT_DEPTH, max_pairs=DEFAULT_MAX_PAIRS, device=None,
                     spacing=None) -> dict:
    """``{"objects", "report", "contacts"}``: ``objects`` is an int32 array of ``vol.shape`` - for every voxel of a separated value the
    lowest voxel index of its object, for every other voxel the root of its component; ``report[str(value)]`` holds ``components``,
    ``separated`` (and ``why`` not), ``basins``, ``pair_rows``, ``adjacent_pairs``, ``merges`` and ``objects``; ``contacts`` holds, per pair of
    touching objects of one value, ``root_a < root_b`` (their ids in ``objects``), ``value``, ``faces`` (z, y, x) and ``neck_squared``, as
    int64 arrays sorted by value, then by the pair.  ``values``: the values to separate (default: every non-zero value present).
    ``spacing`` [sz, sy, sx]: the distance map is that of the weighted grid (``neck_squared`` in its integers ``D``), ``depth`` in voxels of
    the finest axis."""
    shape, zyx, device, v = co.prepare(vol, connectivity, device)
    objects, report, contacts = separate_prepared(v, zyx, device, values, connectivity, depth, max_pairs, lv.grid_of(spacing, zyx)[0])
    objects = objects.cpu().numpy() if lv.is_tensor(objects) else objects
    return {"objects": objects.astype(np.int32, copy=False).reshape(shape), "report": report, "contacts": contacts}


# ---- settings and reporting ------------------------------------------------------------------------------------------------------
def separation_settings(settings) -> dict:
    """the optional predict-settings keys ``measure_separate``, ``measure_separate_values`` (a value or a list; default: every non-zero
    value present), ``measure_separate_depth`` (unit voxels, default 1.0; granular data with rough surfaces usually wants 1 to 2) and
    ``measure_separate_max_pairs`` as arguments, with ``active``: whether ``measure_separate`` asks for work.  Under ``voxel_spacing`` the
    distance map is that of the weighted grid and the result also carries ``voxel_spacing``, ``weights`` and ``unit``; the depth stays in
    voxels of the finest axis."""
    values = getattr(settings, "measure_separate_values", None)
    if values is not None:
        values = _check_values(values, ())
    depth = getattr(settings, "measure_separate_depth", None)
    depth = DEFAULT_DEPTH if depth is None else _check_depth("inf" if isinstance(depth, str) and depth.strip().lower() in ("inf", ".inf") else depth)
    max_pairs = getattr(settings, "measure_separate_max_pairs", None)
    max_pairs = DEFAULT_MAX_PAIRS if max_pairs is None else int(max_pairs)
    if max_pairs < 1:
        raise ValueError("measure_separate_max_pairs must be at least 1")
    out = dict(active=bool(getattr(settings, "measure_separate", False)), values=values, depth=depth, max_pairs=max_pairs)
    grid = lv.spacing_settings(settings)
    if grid is not None:
        out.update(voxel_spacing=list(grid[0]), weights=list(grid[1]), unit=grid[2])
    return out


def contacts_table(contacts: dict, roots, voxel_size=1.0, unit=None) -> dict:
    """The contacts as the columns of ``CONTACT_COLUMNS``: ``id_a`` / ``id_b`` are the ids of the object table whose rows have the roots
    ``roots`` (row + 1; 0 for an object the table does not list), ``contact_area`` = the faces across each axis x the area of a face across
    that axis (``voxel_size``: a scalar or [sz, sy, sx]), ``neck_radius`` = sqrt(``neck_squared``) in voxels - under ``voxel_spacing``, with
    ``unit`` the unit of its grid, ``unit * sqrt(neck_squared)`` in the spacing's units.  The coordination number of
    an object is the number of rows that name it."""
    sz, sy, sx = lv.voxel_size(voxel_size)
    roots = np.asarray(roots, dtype=np.int64)
    order = np.argsort(roots, kind="stable")

    def ids(of):
        if not len(roots):
            return np.zeros(len(of), dtype=np.int64)
        at = np.clip(np.searchsorted(roots[order], of), 0, len(roots) - 1)
        return np.where(roots[order][at] == of, order[at] + 1, 0).astype(np.int64)

    faces = np.asarray(contacts["faces"], dtype=np.int64).reshape(-1, 3)
    neck = np.asarray(contacts["neck_squared"], dtype=np.int64)
    return {"id_a": ids(np.asarray(contacts["root_a"], dtype=np.int64)), "id_b": ids(np.asarray(contacts["root_b"], dtype=np.int64)),
            "value": np.asarray(contacts["value"], dtype=np.int64), "faces_z": faces[:, 0], "faces_y": faces[:, 1], "faces_x": faces[:, 2],
            "contact_area": faces[:, 0] * (sy * sx) + faces[:, 1] * (sz * sx) + faces[:, 2] * (sz * sy), "neck_squared": neck,
            "neck_radius": np.sqrt(neck.astype(np.float64)) if unit is None else float(unit) * np.sqrt(neck.astype(np.float64))}


def separation_text(report: dict) -> str:
    """the per-value report as text, for the log"""
    lines = [f"{'value':>5} {'components':>10} {'basins':>9} {'pair rows':>10} {'merges':>9} {'objects':>9}"]
    for value, row in report.items():
        lines.append(f"{value:>5} {row['components']:>10} {row['basins']:>9} {row['pair_rows']:>10} {row['merges']:>9} {row['objects']:>9}"
                     + ("" if row["separated"] else f"  not separated: {row['why']}"))
    return "\n".join(lines)


def write_contacts(stem, table: dict, settings: dict | None = None, report: dict | None = None) -> list[Path]:
    """``<stem>_object_contacts.csv`` (one row per pair of touching objects, the columns of ``CONTACT_COLUMNS``) and ``.json`` (the
    settings, the per-value report and the same rows)"""
    stem = str(stem)
    written = [Path(stem + "_object_contacts.csv"), Path(stem + "_object_contacts.json")]
    floats = {"contact_area", "neck_radius"}
    rows = [[float(table[c][i]) if c in floats else int(table[c][i]) for c in CONTACT_COLUMNS] for i in range(len(table["id_a"]))]
    with open(written[0], "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(CONTACT_COLUMNS)
        for row in rows:
            w.writerow([repr(x) if isinstance(x, float) else x for x in row])
    with open(written[1], "w") as f:
        doc = {"settings": json_settings(settings), "report": report, "columns": list(CONTACT_COLUMNS), "contacts": rows}
        if settings is not None and "unit" in settings:
            doc["neck_radius"] = "unit * sqrt(neck_squared), in the units of voxel_spacing; neck_squared in the weighted integers of the grid"
        json.dump(doc, f, indent=1)
    return written


def json_settings(settings):
    if settings is None:
        return None
    return {k: (lv.json_number(x) if isinstance(x, float) else x) for k, x in settings.items()}
