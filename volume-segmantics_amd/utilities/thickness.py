"""Local thickness of a label volume: for every voxel of a material the diameter of the largest ball that fits inside the material
and contains the voxel - vessel calibre, pore size, strut and wall thickness.

Definitions (exact integers; include/volseg_hip.h states them for the C ABI).  The volume is ``Z x Y x X`` uint8, x fastest; ``c``
is a label value and ``M`` the voxels equal to ``c``.  ``R(v)``, ``v`` in ``M``, is the squared Euclidean distance in unit voxels to the
nearest voxel IN the volume whose value is not ``c`` (``vs_edt_squared`` with the seeds ``labels != c``): outside the volume is not
background - an object cut by a face of the volume is taken to continue - and an axis of length 1 has no neighbours, so a ``1 x H x
W`` volume is measured in 2-D.  The ball of ``v`` is ``B(v) = {u in the volume : |u - v|^2 < R(v)}``: open, so it holds no seed and lies
inside ``M``.  ``T2(u) = max {R(v) : v in M, u in B(v)}`` on ``M`` and 0 elsewhere, so ``T2 >= R`` on ``M``.  The thickness in physical
units is ``2 s sqrt(T2)``, ``s`` the voxel size.  A value beside which the volume holds no other value has no thickness: its figures
are NaN and its voxels read 0 in the map.  Distances run between voxel centres and that bias is not corrected: a plate ``w`` voxels
wide reads ``w`` for even ``w`` and ``w + 1`` for odd ``w``, a one-voxel line reads 2.

Anisotropic voxels (``voxel_spacing: [sz, sy, sx]``, ``spacing=``): ``label_volume.voxel_grid`` turns the steps into integer weights ``w`` and a
unit ``u``; with ``q = w^2`` the squared distance is the integer ``D(d) = qz dz^2 + qy dy^2 + qx dx^2`` and ``R``, the balls ``{u : D(u - v) <
R(v)}`` and ``T2`` are defined with ``D``; the thickness is ``2 u sqrt(T2)``.  The bias is the same one: a plate ``w`` voxels wide along an
axis of step ``s`` reads ``w s`` or ``(w + 1) s``.  A ball reaches ``isqrt((R - 1) / qz)`` planes and ``isqrt((R - 1) / qy)`` lines, its row has
``m = R - qz dz^2 - qy dy^2`` and the half width ``isqrt((m - 1) / qx)``, and the containment table has seven rows, one per set of axes a
neighbour's offset moves along (``need_table_scaled``).  An isotropic spacing has the weights (1, 1, 1) and runs the unweighted code.

The way there.  (1) Centres: ``v`` is dropped when one of its 26 neighbours ``n = v + delta`` has a ball that contains ``B(v)``: ``R(n) >=
need[class of delta][R(v)]``, ``need[delta][r] = 1 + max {|p - delta|^2 : p in Z^3, |p|^2 < r}``, one row each for a face, an edge and
a corner (``need_table``).  That neighbour's ``R`` is strictly larger, so dropping never changes ``T2``.  (2) Every kept ball is one
x-span per row ``(dz, dy)`` with ``m = R - dz^2 - dy^2 >= 1``: ``[x - h, x + h]``, ``h`` the largest integer with ``h^2 < m``, clipped to
the row.  A span of length ``L`` is recorded on level ``k = floor(log2 L)`` of a sparse table of range maxima - entry ``p`` of level
``k`` covers ``[p, p + 2^k)`` - at its first position and at its last position ``- 2^k + 1``.  (3) The levels are pushed down, ``level[k-1][x]
= max(level[k-1][x], level[k][x], level[k][x - 2^(k-1)])``, and level 0 is the map.

Routes: ``vs_thickness_centres`` / ``_paint`` / ``_resolve`` (csrc/thickness.hip) behind ``vs_edt_squared`` on a GPU; the same pruning and the
same row-span painting in NumPy behind ``surface_distance.squared_distance_transform`` on a host - for small volumes and for parity:
the integers are the same.  Everything reported comes from the integer histogram of ``T2`` over ``M``, in float64, by the same code.

Not here: steps in an irrational ratio or with integer weights above 64, sheared grids, per-object thickness, skeletons or centrelines, a cap on the radius; the background is measured only
when ``thickness_values`` names it."""
from __future__ import annotations

import csv
import json
import logging
import math
from pathlib import Path

import numpy as np

from . import label_volume as lv
from . import surface_distance as sd

INF_R = sd.INF_D2
NEED_MAX_R = 1 << 16          # the longest row of the containment table: a voxel with a larger R is never dropped
LAUNCH_ROWS = 1 << 30         # most row spans (by the bound of the launch's largest ball) one paint launch takes
DEFAULT_MAX_WORK = 8 * 10 ** 12   # row spans: what the measured rate paints in about a minute (profiles/thickness.txt)
HOST_WARN_ROWS = 2 * 10 ** 7  # the host route says so before it paints more row spans than this
FIGURES = ("mean", "std", "min", "max", "median", "p5", "p95", "largest_inscribed_diameter")
_OFFSETS = [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dz, dy, dx) != (0, 0, 0)]
_need_cache: dict = {}


# ---- integers ----------------------------------------------------------------------------------------------------------------------
def _isqrt(v) -> np.ndarray:
    """the largest h with h^2 <= v, element by element (int64, exact)"""
    v = np.asarray(v, dtype=np.int64)
    h = np.floor(np.sqrt(v.astype(np.float64))).astype(np.int64)
    h -= h * h > v
    h += (h + 1) * (h + 1) <= v
    return h


def table_levels(x: int, max_r: int, qx: int = 1) -> int:
    """K = bit_length(min(2 h + 1, X)), h the largest integer with qx h^2 < max_r: the levels of the sparse table"""
    return int(min(2 * math.isqrt((int(max_r) - 1) // int(qx)) + 1, int(x))).bit_length()


def need_table(max_r: int) -> np.ndarray:
    """(3, min(max_r, NEED_MAX_R) + 1) uint32: ``need[j - 1][r]`` = 1 + the largest ``|p - delta|^2`` over the lattice points ``|p|^2 < r``,
    ``delta`` with ``j`` non-zero components of size 1 - the least ``R`` of a neighbour at ``delta`` whose ball contains the ball of squared
    radius ``r``.  Row 0 is never read at ``r = 0``.  By symmetry the maximum is taken over ``p = (a >= b >= c >= 0)`` placed against
    ``delta``: ``|p|^2 + 2 (a | a + b | a + b + c) + j``; the points are sorted by ``|p|^2`` and a prefix maximum is taken.  Cached."""
    top = min(int(max_r), NEED_MAX_R)
    have = _need_cache.get("table")
    if have is None or have.shape[1] < top + 1:
        h = math.isqrt(max(top - 1, 0))
        a = np.arange(h + 1, dtype=np.int64)
        a, b, c = np.meshgrid(a, a, a, indexing="ij", sparse=True)
        ordered = (a >= b) & (b >= c)
        s = (a * a + b * b + c * c)[ordered]
        lead = [np.broadcast_to(t, ordered.shape)[ordered] for t in (a, a + b, a + b + c)]
        inside = s < top
        order = np.argsort(s[inside], kind="stable")
        s = s[inside][order]
        below = np.searchsorted(s, np.arange(top + 1), side="left") - 1          # the last point with |p|^2 < r; -1 only at r = 0
        table = np.zeros((3, top + 1), dtype=np.uint32)
        for j in range(3):
            best = np.maximum.accumulate((s + 2 * lead[j][inside][order]))
            table[j] = np.where(below >= 0, best[np.maximum(below, 0)] + (j + 1) + 1, 0)
        _need_cache["table"] = have = table
    return np.ascontiguousarray(have[:, :top + 1])


NEED_MAX_LEN = 1 << 22        # the longest row of the weighted table, whatever the weights: 7 rows of 16 MiB


def _subset_row(dz, dy, dx) -> int:
    """the row of the weighted containment table for a neighbour offset: the set of axes on which it is non-zero, 4 [z] + 2 [y] + [x] - 1"""
    return 4 * (dz != 0) + 2 * (dy != 0) + (dx != 0) - 1


def need_table_scaled(max_r: int, weights) -> np.ndarray:
    """(7, top + 1) uint32, ``top = min(max_r, NEED_MAX_R min(q), NEED_MAX_LEN)``: ``need[row][r] = 1 + max {D(p) + sum over the axes i of the
    row of q_i (2 |p_i| + 1) : p in Z^3, D(p) < r}``, ``D(p) = qz pz^2 + qy py^2 + qx px^2``, ``q = w^2``, one row per non-empty set of axes on which
    a neighbour's offset is non-zero (``_subset_row``) - the least ``R`` of that neighbour whose ball contains the ball of squared radius
    ``r``.  The table ends where, in weighted units, ``NEED_MAX_R`` ends on the finest axis, so that it covers as many coarse voxels as the
    unweighted table covers voxels; a voxel beyond its end is kept.  The maximum runs over ``p >= 0`` placed against the offset; the
    points are sorted by ``D`` and a prefix maximum is taken.  With weights (1, 1, 1) rows 0, 2 and 6 are the rows of ``need_table``.  The last grid's table is cached."""
    w = tuple(int(x) for x in weights)
    q = [x * x for x in w]
    top = min(int(max_r), NEED_MAX_R * min(q), NEED_MAX_LEN)
    have = _need_cache.get("weighted", (None, None))
    have = have[1] if have[0] == w else None                           # one weighted table is kept: the last grid's
    if have is None or have.shape[1] < top + 1:
        axes = [np.arange(math.isqrt(max(top - 1, 0) // qi) + 1, dtype=np.int64) for qi in q]
        pz, py, px = np.meshgrid(*axes, indexing="ij", sparse=True)
        s = q[0] * pz * pz + q[1] * py * py + q[2] * px * px
        inside = s < top
        lead = [np.broadcast_to(qi * (2 * t + 1), s.shape)[inside] for qi, t in zip(q, (pz, py, px))]
        s = s[inside]
        order = np.argsort(s, kind="stable")
        s = s[order]
        below = np.searchsorted(s, np.arange(top + 1), side="left") - 1          # the last point with D(p) < r; -1 only at r = 0
        table = np.zeros((7, top + 1), dtype=np.uint32)
        for row in range(7):
            extra = sum(lead[i] for i in range(3) if (row + 1) & (4 >> i))
            best = np.maximum.accumulate(s + extra[order])
            table[row] = np.where(below >= 0, best[np.maximum(below, 0)] + 1, 0)
        _need_cache["weighted"] = (w, table)
        have = table
    return np.ascontiguousarray(have[:, :top + 1])


def _ball_rows(z, y, r, zyx, weights=lv.UNIT_WEIGHTS):
    """per centre the rows (dz, dy) of the bounding rectangle of its ball that lie in the volume - what the paint pass runs through"""
    r = np.asarray(r, dtype=np.int64)
    hz, hy = _isqrt((r - 1) // weights[0] ** 2), _isqrt((r - 1) // weights[1] ** 2)
    nz = np.minimum(z + hz, zyx[0] - 1) - np.maximum(z - hz, 0) + 1
    ny = np.minimum(y + hy, zyx[1] - 1) - np.maximum(y - hy, 0) + 1
    return nz * ny


def _check_value(value) -> int:
    value = int(value)
    if not 0 <= value <= 255:
        raise ValueError(f"value {value} is not a uint8 value")
    return value


def _check_work(rows: int, max_work, value: int) -> None:
    if max_work is not None and rows > max_work:
        raise ValueError(f"the local thickness of value {value} paints {rows} row spans, more than thickness_max_work = {int(max_work)}: raise "
                         f"the key, or leave the value out of thickness_values")


# ---- host route ------------------------------------------------------------------------------------------------------------------
def centres_host(r: np.ndarray, need: np.ndarray | None) -> np.ndarray:
    """ascending voxel indices of the centres of ``r`` (Z, Y, X): ``r > 0`` and no neighbour's ball contains the voxel's; ``need`` None keeps
    all.  ``need`` of 3 rows is ``need_table`` (a face, an edge, a corner), of 7 rows ``need_table_scaled`` (the axes of the offset)."""
    r = np.asarray(r).astype(np.int64)
    keep = r > 0
    if need is not None and need.shape[1]:
        z, y, x = r.shape
        length = need.shape[1]
        droppable = keep & (r < length)
        at = np.minimum(r, length - 1)
        padded = np.pad(r, 1, constant_values=0)            # a neighbour outside the volume contains nothing
        for dz, dy, dx in _OFFSETS:
            row = _subset_row(dz, dy, dx) if need.shape[0] == 7 else (dz != 0) + (dy != 0) + (dx != 0) - 1
            neighbour = padded[1 + dz:1 + dz + z, 1 + dy:1 + dy + y, 1 + dx:1 + dx + x]
            keep &= ~(droppable & (neighbour >= need[row].astype(np.int64)[at]))
    return np.flatnonzero(keep)


def paint_host(r: np.ndarray, centres: np.ndarray, levels: int, weights=lv.UNIT_WEIGHTS) -> np.ndarray:
    """(levels, n) uint32: the sparse table after the row spans of the balls of ``centres`` went in (before it is resolved)"""
    qz, qy, qx = (int(w) ** 2 for w in weights)
    zyx = r.shape
    big_z, big_y, big_x = zyx
    table = np.zeros((levels, r.size), dtype=np.uint32)
    if len(centres) == 0:
        return table
    z, y, x = (c.astype(np.int64) for c in np.unravel_index(centres, zyx))
    rv = r.reshape(-1)[centres].astype(np.int64)
    reach_z, reach_y = int(_isqrt((rv.max() - 1) // qz)), int(_isqrt((rv.max() - 1) // qy))
    for dz in range(-min(reach_z, big_z - 1), min(reach_z, big_z - 1) + 1):
        for dy in range(-min(reach_y, big_y - 1), min(reach_y, big_y - 1) + 1):
            m = rv - (qz * dz * dz + qy * dy * dy)
            zz, yy = z + dz, y + dy
            ok = (m >= 1) & (zz >= 0) & (zz < big_z) & (yy >= 0) & (yy < big_y)
            if not ok.any():
                continue
            h = _isqrt((m[ok] - 1) // qx)                    # the largest h with qx h^2 < m
            first, last = np.maximum(x[ok] - h, 0), np.minimum(x[ok] + h, big_x - 1)
            k = np.frexp((last - first + 1).astype(np.float64))[1] - 1          # floor(log2 L), exact
            row = (zz[ok] * big_y + yy[ok]) * big_x
            value = rv[ok].astype(np.uint32)
            np.maximum.at(table, (k, row + first), value)
            np.maximum.at(table, (k, row + last - (np.int64(1) << k) + 1), value)
    return table


def resolve_host(table: np.ndarray, x: int) -> np.ndarray:
    """the levels pushed down, in place: level 0 is then the painted map"""
    for k in range(table.shape[0] - 1, 0, -1):
        hi, lo, half = table[k].reshape(-1, x), table[k - 1].reshape(-1, x), 1 << (k - 1)
        np.maximum(lo, hi, out=lo)
        np.maximum(lo[:, half:], hi[:, :x - half], out=lo[:, half:])
    return table


def _need(max_r: int, weights) -> np.ndarray:
    return need_table(max_r) if tuple(weights) == lv.UNIT_WEIGHTS else need_table_scaled(max_r, weights)


def _value_host(v: np.ndarray, value: int, t2: np.ndarray, max_work, prune: bool = True, weights=lv.UNIT_WEIGHTS) -> dict:
    member = v == value
    voxels = int(member.sum())
    info = dict(voxels=voxels, max_r=None, centres=0, row_spans=0, levels=0, workspace_bytes=0)
    if voxels == 0 or voxels == v.size:
        return info
    unit = tuple(weights) == lv.UNIT_WEIGHTS
    r = sd.squared_distance_transform(~member, device="cpu").reshape(v.shape) if unit else sd.edt_host(~member, weights)
    max_r = int(r.max())
    centres = centres_host(r, _need(max_r, weights) if prune else None)
    z, y, _ = np.unravel_index(centres, v.shape)
    rows = int(_ball_rows(z.astype(np.int64), y.astype(np.int64), r.reshape(-1)[centres], v.shape, weights).sum())
    _check_work(rows, max_work, value)
    if rows > HOST_WARN_ROWS:
        logging.warning(f"local thickness of value {value} on the host: {len(centres)} centres paint {rows} row spans in NumPy - this route is for "
                        f"small volumes; a GPU paints them in csrc/thickness.hip")
    levels = table_levels(v.shape[2], max_r, weights[2] ** 2)
    table = resolve_host(paint_host(r, centres, levels, weights), v.shape[2])
    t2[member] = table[0].reshape(v.shape)[member]
    info.update(max_r=max_r, centres=int(len(centres)), row_spans=rows, levels=levels, workspace_bytes=4 * levels * v.size)
    return info


# ---- device route ----------------------------------------------------------------------------------------------------------------
def _max_u32(t, zyx, weights=lv.UNIT_WEIGHTS) -> int:
    """the largest element of an int32 tensor that holds uint32 values: squared distances of a ``zyx`` volume under ``weights``"""
    if sum((w * (e - 1)) ** 2 for w, e in zip(weights, zyx)) < 1 << 31:
        return int(t.max())
    import torch
    return int((t.to(torch.int64) & 0xFFFFFFFF).max())


def launch_plan(radii, counts, zyx, launch_rows: int = LAUNCH_ROWS, weights=lv.UNIT_WEIGHTS) -> list[tuple[int, int, int]]:
    """[(begin, end, largest R)] over a centre list in groups of falling size, ``radii`` the largest R of each group and ``counts`` its
    centres: every launch takes at most ``launch_rows`` row spans by the bound of its first group's largest ball, and at least 64 centres"""
    ends = np.cumsum(np.asarray(counts, dtype=np.int64))
    total, plan, begin = int(ends[-1]) if len(ends) else 0, [], 0
    while begin < total:
        largest = int(radii[int(np.searchsorted(ends, begin, side="right"))])
        planes, lines = (2 * math.isqrt((largest - 1) // int(w) ** 2) + 1 for w in weights[:2])
        bound = min(planes, zyx[0]) * min(lines, zyx[1])
        end = min(total, begin + max(64, launch_rows // bound))
        plan.append((begin, end, largest))
        begin = end
    return plan


def order_centres(r, centres, zyx, max_r: int, weights=lv.UNIT_WEIGHTS):
    """(the centre list as it is painted, its launch plan): in groups by floor(log4 R), the largest first, and in voxel order inside a
    group.  A batch of the paint kernel then holds balls of one size class, which is what sizes its grid, and neighbours in the
    list are neighbours in the volume, whose rows share cache lines: on the vessels volume this order paints 2.7 x as fast as the
    list sorted by R alone (profiles/thickness.txt).  The order changes no integer: the table holds maxima."""
    import torch
    centres, _ = torch.sort(centres)
    radii = torch.index_select(r, 0, centres).to(torch.int64) & 0xFFFFFFFF
    bounds = torch.tensor([4 ** k for k in range(1, 17)], dtype=torch.int64, device=r.device)
    group = torch.bucketize(radii, bounds, right=True).to(torch.uint8)                  # floor(log4 R), 0 .. 15, by integer compares
    _, order = torch.sort(group, descending=True, stable=True)
    counts = torch.bincount(group.to(torch.int64), minlength=16).cpu().numpy()[::-1]     # the largest group first
    tops = [min(4 ** (g + 1) - 1, int(max_r)) for g in range(15, -1, -1)]
    present = counts > 0
    return centres[order].contiguous(), launch_plan(np.asarray(tops)[present], counts[present], zyx, LAUNCH_ROWS, weights)


def _value_device(v, zyx, value: int, t2, max_work, keep_table: bool = False, weights=lv.UNIT_WEIGHTS) -> dict:
    """one value on the device: ``t2`` (n int32 on the device, uint32 bits) receives T2 at the voxels of the value.  Under ``weights``
    other than (1, 1, 1) the ``_scaled`` entry points run, which take the weights after the extents, with the 7-row table."""
    import torch
    from .. import _lib
    w = () if tuple(weights) == lv.UNIT_WEIGHTS else tuple(int(x) for x in weights)
    entry = lambda name: getattr(_lib.lib, name + "_scaled" if w else name)          # noqa: E731
    device, n = v.device, v.numel()
    member = v == value
    voxels = int(member.sum())
    info = dict(voxels=voxels, max_r=None, centres=0, row_spans=0, levels=0, workspace_bytes=0)
    if voxels == 0 or voxels == n:
        return info
    edt_bytes = int(_lib.lib.vs_edt_workspace_bytes(*zyx))
    lv.require_memory(device, n + 4 * n + edt_bytes + 4 * voxels + 64, f"the distance transform and the centres of value {value} of a {tuple(zyx)} volume")
    seeds = (~member).to(torch.uint8)
    r = torch.empty(n, dtype=torch.int32, device=device)
    sd.edt_device(seeds, zyx, r, torch.empty(edt_bytes, dtype=torch.uint8, device=device), weights)
    del seeds
    max_r = _max_u32(r, zyx, weights)                                     # one sync: the table's length and the levels depend on it
    need = torch.from_numpy(_need(max_r, weights).view(np.int32)).to(device)
    centres = torch.empty(voxels, dtype=torch.int32, device=device)
    totals = torch.empty(2, dtype=torch.int64, device=device)
    with torch.cuda.device(device):
        _lib.check(entry("vs_thickness_centres")(_lib.ptr(r), *zyx, *w, _lib.ptr(need), need.shape[1], _lib.ptr(centres), voxels, _lib.ptr(totals),
                                                 _lib.stream_ptr()))
        count, rows = (int(t) for t in totals.cpu())
        if count > voxels:
            raise RuntimeError(f"value {value}: {count} centres among {voxels} voxels")
        _check_work(rows, max_work, value)
        levels = table_levels(zyx[2], max_r, int(weights[2]) ** 2)
        work_bytes = int(entry("vs_thickness_workspace_bytes")(*zyx, *w, max_r))
        lv.require_memory(device, work_bytes + 16 * count, f"the {levels} levels of the thickness table of a {tuple(zyx)} volume")
        work = torch.empty(work_bytes, dtype=torch.uint8, device=device)
        centres, plan = order_centres(r, centres[:count], zyx, max_r, weights)
        for i, (begin, end, largest) in enumerate(plan):
            _lib.check(entry("vs_thickness_paint")(_lib.ptr(r), *zyx, *w, centres.data_ptr() + 4 * begin, end - begin, largest, max_r, _lib.ptr(work),
                                                   work_bytes, int(i == 0), _lib.stream_ptr()))
        if not plan:
            work.zero_()
        _lib.check(entry("vs_thickness_resolve")(_lib.ptr(v), *zyx, *w, value, max_r, _lib.ptr(work), work_bytes, _lib.ptr(t2), _lib.stream_ptr()))
    info.update(max_r=max_r, centres=count, row_spans=rows, levels=levels, workspace_bytes=work_bytes, launches=len(plan))
    if keep_table:
        info.update(table=work.view(torch.int32).reshape(levels, n), centre_list=centres, r=r)
    return info


def _histogram_device(v, value: int, t2, zyx, weights=lv.UNIT_WEIGHTS) -> np.ndarray:
    import torch
    from .. import _lib
    scaled = tuple(weights) != lv.UNIT_WEIGHTS
    bins = None if scaled else sd.histogram_bins(zyx)
    lv.require_memory(v.device, v.numel() + (9 * v.numel() if scaled else 8 * bins), f"the thickness histogram of a {tuple(zyx)} volume")
    mask = (v == value).to(torch.uint8)
    if scaled:                                 # the bins follow the largest value present, not the bound of the shape, which the weights raise
        bins = sd.bins_present(sd.masked_max_device(mask, t2))
    hist = torch.empty(bins, dtype=torch.int64, device=v.device)
    with torch.cuda.device(v.device):
        _lib.check(_lib.lib.vs_surface_distance_histogram(_lib.ptr(mask), _lib.ptr(t2), v.numel(), bins, _lib.ptr(hist), _lib.stream_ptr()))
    return _trim(hist.cpu().numpy())


def _trim(hist: np.ndarray) -> np.ndarray:
    used = np.flatnonzero(hist)
    return np.ascontiguousarray(hist[:int(used[-1]) + 1 if len(used) else 1]).astype(np.int64)


# ---- public: the integers --------------------------------------------------------------------------------------------------------
def _labels(vol, device):
    """(shape, zyx, device or None, the volume as a host (Z, Y, X) array or a flat aligned device tensor)"""
    sd.histogram_bins(tuple(vol.shape))         # raises where a squared distance does not fit
    if int(np.prod(lv.zyx(tuple(vol.shape)))) >= 1 << 31:
        raise ValueError(f"a volume of shape {tuple(vol.shape)} has 2^31 voxels or more: centres are int32 voxel indices")
    return lv.prepare(vol, device, lambda zyx, resident: (0 if resident else int(np.prod(zyx))) + 4 * int(np.prod(zyx)), "thickness map")


def _run(vol, values, device, max_work, want_histograms: bool, spacing=None):
    """(shape, T2 as a host uint32 array of vol.shape, {value: info}) - every value into one map"""
    shape, zyx, device, v = _labels(vol, device)
    weights, _ = lv.grid_of(spacing, zyx)
    infos = {}
    if device is None:
        t2 = np.zeros(zyx, dtype=np.uint32)
        for value in values:
            infos[value] = _value_host(v, value, t2, max_work, weights=weights)
            if want_histograms:
                infos[value]["histogram"] = _trim(np.bincount(t2[v == value].astype(np.int64), minlength=1))
        return shape, zyx, t2.reshape(shape), infos
    import torch
    t2 = torch.zeros(v.numel(), dtype=torch.int32, device=device)
    for value in values:
        infos[value] = _value_device(v, zyx, value, t2, max_work, weights=weights)
        if want_histograms:
            infos[value]["histogram"] = _histogram_device(v, value, t2, zyx, weights)
    return shape, zyx, t2.cpu().numpy().view(np.uint32).reshape(shape), infos


def local_thickness_squared(vol, value, device=None, max_work=None, spacing=None) -> np.ndarray:
    """uint32 array of ``vol.shape``: ``T2`` of the voxels equal to ``value``, 0 elsewhere - and everywhere when the volume holds no other
    value.  The HIP kernels where ``device`` (default: the volume's, else the current GPU) is one, the host route otherwise: the same
    integers.  ``max_work``: refuse (ValueError) when the balls would paint more row spans than this.  ``spacing`` [sz, sy, sx]: ``T2`` in
    the weighted integers ``D`` of ``label_volume.voxel_grid(spacing)`` - the thickness is ``2 unit sqrt(T2)``."""
    return _run(vol, [_check_value(value)], device, max_work, False, spacing)[2]


def thickness_histogram(t2, vol, value, device=None, spacing=None) -> np.ndarray:
    """int64 array: ``hist[k]`` = the voxels of ``vol`` equal to ``value`` whose ``t2`` is ``k``, trailing zeros trimmed
    (``vs_surface_distance_histogram`` over the mask ``vol == value`` on a GPU, ``bincount`` on a host).  ``spacing``: the one ``t2`` was
    computed with - its values then exceed the unit-voxel bound of the shape, and the bins follow the largest value present."""
    value = _check_value(value)
    if tuple(t2.shape) != tuple(vol.shape):
        raise ValueError(f"the thickness map has shape {tuple(t2.shape)} but the volume has shape {tuple(vol.shape)}")
    _, zyx, device, v = _labels(vol, device)
    weights, _ = lv.grid_of(spacing, zyx)
    if device is None:
        return _trim(np.bincount(lv.to_host(t2).reshape(zyx)[v == value].astype(np.int64), minlength=1))
    import torch
    t = t2 if lv.is_tensor(t2) else torch.from_numpy(np.ascontiguousarray(t2).view(np.int32))
    t = t.to(device).contiguous().reshape(-1)
    return _histogram_device(v, value, t if t.data_ptr() % 16 == 0 else t.clone(), zyx, weights)


# ---- public: the figures -----------------------------------------------------------------------------------------------------------
def thickness_scores_from_histogram(hist, max_r=None, voxel_size: float = 1.0) -> dict:
    """The figures of one value in float64 from the integer histogram of ``T2`` alone: ``voxels``; ``mean``, ``std`` (population), ``min``,
    ``max``, ``median``, ``p5`` and ``p95`` (NumPy's linear interpolation) of the thickness ``2 s sqrt(T2)`` weighted by voxel - which is
    volume-weighted; ``largest_inscribed_diameter`` = ``2 s sqrt(max R)``.  ``max_r`` None - no thickness - gives NaN for all but ``voxels``."""
    hist = np.asarray(hist, dtype=np.int64).reshape(-1)
    scale = float(voxel_size)
    out = {"voxels": int(hist.sum())}
    out.update({name: float("nan") for name in FIGURES})
    used = np.flatnonzero(hist)
    if max_r is None or len(used) == 0:
        return out
    counts, total = hist[used], int(hist.sum())
    d = 2.0 * scale * np.sqrt(used.astype(np.float64))
    mean = float((counts * d).sum()) / total
    out.update(mean=mean, std=math.sqrt(float((counts * (d - mean) ** 2).sum()) / total), min=float(d[0]), max=float(d[-1]),
               median=lv.percentile_from_counts(d, counts, 50.0), p5=lv.percentile_from_counts(d, counts, 5.0),
               p95=lv.percentile_from_counts(d, counts, 95.0), largest_inscribed_diameter=2.0 * scale * math.sqrt(float(max_r)))
    return out


# ---- settings and reporting ------------------------------------------------------------------------------------------------------
def thickness_settings(settings) -> dict:
    """the optional predict-settings keys ``thickness_map``, ``thickness_values`` (a list; default None: every non-zero value present),
    ``thickness_voxel_size`` (ONE positive number; default ``measure_voxel_size`` where that is a single number, else 1.0; an error beside
    ``voxel_spacing``, under which the result also carries ``voxel_spacing``, ``weights`` and ``unit``, and ``voxel_size`` is the unit), ``thickness_save_volume`` and ``thickness_max_work`` (row spans) as arguments, with ``active``: whether
    ``thickness_map`` asks for work"""
    values = getattr(settings, "thickness_values", None)
    if values is not None:
        values = sorted({int(v) for v in (values if isinstance(values, (list, tuple)) else [values])})
        if any(not 0 <= v <= 255 for v in values):
            raise ValueError(f"thickness_values {values}: every one is a uint8 value")
    grid = lv.spacing_settings(settings, "thickness_voxel_size")
    size = getattr(settings, "thickness_voxel_size", None)
    if grid is not None:
        size = grid[2]               # the unit of the grid: the thickness is 2 u sqrt(T2) with T2 in weighted integers
    elif size is None:
        size = getattr(settings, "measure_voxel_size", None)
        size = 1.0 if size is None or np.asarray(size).size != 1 else size
    if np.asarray(size).size != 1:
        raise ValueError(f"thickness_voxel_size {size!r}: it is one positive number - the distance transform is isotropic, anisotropic voxels "
                         f"are not measured")
    size = lv.voxel_size(size)[0]
    max_work = getattr(settings, "thickness_max_work", None)
    max_work = DEFAULT_MAX_WORK if max_work is None else int(max_work)
    if max_work < 1:
        raise ValueError("thickness_max_work must be at least 1")
    out = dict(active=bool(getattr(settings, "thickness_map", False)), values=values, voxel_size=size,
               save_volume=bool(getattr(settings, "thickness_save_volume", False)), max_work=max_work)
    if grid is not None:
        out.update(voxel_spacing=list(grid[0]), weights=list(grid[1]), unit=grid[2])
    return out


def _present(vol) -> list[int]:
    if lv.is_tensor(vol):
        import torch
        return [int(c) for c in torch.unique(vol).cpu().tolist()]
    return [int(c) for c in np.unique(np.asarray(vol)).tolist()]


def thickness_label_volume(vol, settings, device=None) -> dict:
    """``local_thickness_squared`` of every value and its figures with the settings keys: ``{"settings", "shape", "squared": T2 (uint32,
    the values share it), "values": {value: {"figures", "histogram", "max_squared_radius", "centres", "row_spans", "levels",
    "workspace_bytes"}}, "volume": the float32 thicknesses with thickness_save_volume, else None}``.  Runs whether or not
    ``thickness_map`` is set: calling is the request."""
    t = thickness_settings(settings)
    values = t["values"]
    if values is None:
        values = [c for c in _present(lv.strict_u8(vol)) if c != 0]
    _, zyx, squared, infos = _run(vol, values, device, t["max_work"], True, t.get("voxel_spacing"))
    report = {}
    for value in values:
        info = infos[value]
        report[value] = {"figures": thickness_scores_from_histogram(info["histogram"], info["max_r"], t["voxel_size"]), "histogram": info["histogram"],
                         "max_squared_radius": info["max_r"], "centres": info["centres"], "row_spans": info["row_spans"], "levels": info["levels"],
                         "workspace_bytes": info["workspace_bytes"]}
    volume = (2.0 * t["voxel_size"] * np.sqrt(squared.astype(np.float64))).astype(np.float32) if t["save_volume"] else None
    return {"settings": t, "shape": [int(s) for s in zyx], "squared": squared, "values": report, "volume": volume}


def thickness_summary_text(kept: dict) -> str:
    """the per-value figures as text, for the log"""
    lines = [f"{'value':>5} {'voxels':>12} {'mean':>10} {'std':>10} {'min':>10} {'p5':>10} {'median':>10} {'p95':>10} {'max':>10} {'inscribed':>10} "
             f"{'centres':>11} {'row spans':>13}"]
    for value, row in kept["values"].items():
        f = row["figures"]
        lines.append(f"{value:>5} {f['voxels']:>12} {f['mean']:>10.4f} {f['std']:>10.4f} {f['min']:>10.4f} {f['p5']:>10.4f} {f['median']:>10.4f} "
                     f"{f['p95']:>10.4f} {f['max']:>10.4f} {f['largest_inscribed_diameter']:>10.4f} {row['centres']:>11} {row['row_spans']:>13}")
    lines.append(f"thickness = 2 x {kept['settings']['voxel_size']:g} x sqrt(T2), weighted by voxel; distances between voxel centres (a plate w voxels "
                 f"wide reads w for even w and w + 1 for odd w)")
    return "\n".join(lines)


def write_thickness(stem, kept: dict) -> list[Path]:
    """``<stem>_thickness.csv`` (one row per value: the voxels, the figures, the centres and the row spans) and ``<stem>_thickness.json``:
    the settings, the shape and per value the same with the largest squared radius and the non-zero part of the histogram of ``T2``
    - the integers every figure comes from; NaN is written as null.  (The float32 volume of ``thickness_save_volume`` is the caller's
    to save: it knows the chunking.)"""
    stem = str(stem)
    written = [Path(stem + "_thickness.csv"), Path(stem + "_thickness.json")]
    with open(written[0], "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(("value", "voxels") + FIGURES + ("centres", "row_spans"))
        for value, row in kept["values"].items():
            w.writerow([value, row["figures"]["voxels"]] + [repr(float(row["figures"][name])) for name in FIGURES] + [row["centres"], row["row_spans"]])
    doc = {"settings": kept["settings"], "shape": kept["shape"], "values": {}}
    for value, row in kept["values"].items():
        used = np.flatnonzero(row["histogram"])
        entry = {"voxels": row["figures"]["voxels"]}
        entry.update({name: lv.json_number(row["figures"][name]) for name in FIGURES})
        entry.update(max_squared_radius=row["max_squared_radius"], centres=row["centres"], row_spans=row["row_spans"],
                     histogram={"squared_thickness": used.tolist(), "count": row["histogram"][used].tolist()})
        doc["values"][str(value)] = entry
    with open(written[1], "w") as f:
        json.dump(doc, f, indent=1)
    return written
