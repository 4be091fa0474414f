"""Measurements of the objects of a label volume: per connected component its voxels, centroid, bounding box, face-count surface,
principal axes and whether it touches the boundary - what people segment vessels, pores, grains or cells for.

Definitions.  Volumes, connectivity, components and roots are those of ``utilities/components.py``.  One table row per MEASURED
component: a component is left out when it has fewer than ``min_voxels`` voxels, or when its value is ``background`` and the
background is not asked for; the components left out are counted per value (``not_listed_objects`` / ``not_listed_voxels``).  Rows
are ordered by label value ascending, then root ascending, and the object id of a row is row + 1.  A row holds the 20 exact
integers of ``FIELDS``: voxels; sum z, y, x; sum z^2, y^2, x^2; sum zy, zx, yx; min / max z, y, x; exposed faces across z, y, x;
touches.  An exposed face of a voxel is a face neighbour along that axis whose value differs or which lies outside the volume; an
axis of length 1 has no faces (the convention of ``label_surface`` and ``component_table``).  ``touches`` is that of
``vs_component_sizes``.  Every sum stays below n (E - 1)^2, E the longest extent: a volume for which that does not fit int64 is
refused.

All routes give the same integers: ``vs_component_moments`` (csrc/measure.hip) on the roots of ``vs_label_components`` on a GPU, sorted
``np.add.reduceat`` sums in int64 on a host.  Every derived figure (``object_table``) is computed in float64 from those integers
alone, by the same code, so the derived figures of the routes agree bit for bit."""
from __future__ import annotations

import csv
import json
import math
from pathlib import Path

import numpy as np

from . import components as co
from . import label_volume as lv

FIELDS = ("voxels", "sum_z", "sum_y", "sum_x", "sum_zz", "sum_yy", "sum_xx", "sum_zy", "sum_zx", "sum_yx",
          "min_z", "max_z", "min_y", "max_y", "min_x", "max_x", "faces_z", "faces_y", "faces_x", "touches_border")      # csrc/measure.hip kFields
F = {name: i for i, name in enumerate(FIELDS)}
SUM_LIMIT = 1 << 63


# ---- arguments -------------------------------------------------------------------------------------------------------------------
def _check_sums_fit(shape) -> None:
    zyx = lv.zyx(shape)
    n, longest = zyx[0] * zyx[1] * zyx[2], max(zyx)
    if n * (longest - 1) ** 2 >= SUM_LIMIT:
        raise ValueError(f"a volume of shape {tuple(shape)} can hold a sum of squared coordinates of {n} x {longest - 1}^2, which does not "
                         f"fit int64: it cannot be measured")


def _arguments(min_voxels, background):
    min_voxels, background = int(min_voxels), int(background)
    if min_voxels < 1:
        raise ValueError("min_voxels must be at least 1")
    if not 0 <= background <= 255:
        raise ValueError(f"background {background} is not a uint8 value")
    return min_voxels, background


# ---- host route ------------------------------------------------------------------------------------------------------------------
def _select_host(sizes, values, min_voxels: int, background: int, include_background: bool):
    """(keep mask over the components, not-listed objects and voxels per value)"""
    keep = sizes >= min_voxels
    if not include_background:
        keep &= values != background
    objects = np.bincount(values[~keep], minlength=256).astype(np.int64)
    voxels = np.zeros(256, dtype=np.int64)
    np.add.at(voxels, values[~keep], sizes[~keep])
    return keep, objects, voxels


def _exposed_host(vol: np.ndarray, axis: int) -> np.ndarray:
    """per voxel the exposed faces across `axis` (0, 1 or 2): shifted comparisons on a padded copy.  `vol` holds label values, or - the
    id-based form - the object ids of a labelling: a face neighbour with another id is then exposed, whatever its value"""
    if vol.shape[axis] == 1:
        return np.zeros(vol.shape, dtype=np.uint8)
    pad = [(0, 0)] * 3
    pad[axis] = (1, 1)
    padded = np.pad(vol.astype(np.int16 if vol.dtype == np.uint8 else np.int64), pad, constant_values=-1)
    lo, hi = [slice(None)] * 3, [slice(None)] * 3
    lo[axis], hi[axis] = slice(0, -2), slice(2, None)
    return (padded[tuple(lo)] != vol).astype(np.uint8) + (padded[tuple(hi)] != vol).astype(np.uint8)


def _table_host(vol: np.ndarray, comp: np.ndarray, row_of_root: np.ndarray, rows: int, by_id: bool = False) -> np.ndarray:
    """the (rows, 20) table by sorting the measured voxels by row and summing each stretch in int64; `by_id`: exposed faces from the
    ids of `comp` (separated objects) instead of the values of `vol`"""
    table = np.zeros((rows, len(FIELDS)), dtype=np.int64)
    if rows == 0:
        return table
    row_of_voxel = row_of_root[comp.reshape(-1)]
    measured = np.flatnonzero(row_of_voxel >= 0)
    order = measured[np.argsort(row_of_voxel[measured], kind="stable")]
    starts = np.searchsorted(row_of_voxel[order], np.arange(rows))
    z, y, x = (c.astype(np.int64) for c in np.unravel_index(order, vol.shape))
    ones = np.ones(order.size, dtype=np.int64)
    for name, what in (("voxels", ones), ("sum_z", z), ("sum_y", y), ("sum_x", x), ("sum_zz", z * z), ("sum_yy", y * y), ("sum_xx", x * x),
                       ("sum_zy", z * y), ("sum_zx", z * x), ("sum_yx", y * x)):
        table[:, F[name]] = np.add.reduceat(what, starts)
    for axis, (letter, coord) in enumerate((("z", z), ("y", y), ("x", x))):
        table[:, F["min_" + letter]] = np.minimum.reduceat(coord, starts)
        table[:, F["max_" + letter]] = np.maximum.reduceat(coord, starts)
        table[:, F["faces_" + letter]] = np.add.reduceat(_exposed_host(comp.reshape(vol.shape) if by_id else vol, axis).reshape(-1)[order].astype(np.int64), starts)
    table[:, F["touches_border"]] = np.maximum.reduceat(lv.touch_mask(vol.shape).reshape(-1)[order].astype(np.int64), starts)
    return table


def _measure_host(vol: np.ndarray, connectivity: int, min_voxels: int, background: int, include_background: bool, want_ids: bool,
                  separate: dict | None = None):
    separation = None
    if separate is None:
        comp = co.label_components(vol, connectivity, device="cpu")
    else:
        from . import separation as sp
        comp, report, contacts = sp.separate_prepared(vol, vol.shape, None, separate["values"], connectivity, separate["depth"], separate["max_pairs"],
                                                             separate.get("weights", lv.UNIT_WEIGHTS))
        separation = dict(report=report, contacts=contacts)
    flat_c = comp.reshape(-1)
    size = np.bincount(flat_c, minlength=flat_c.size)
    roots = np.flatnonzero(size).astype(np.int64)
    sizes, values = size[roots].astype(np.int64), vol.reshape(-1)[roots].astype(np.int64)
    keep, objects, voxels = _select_host(sizes, values, min_voxels, background, include_background)
    order = np.lexsort((roots[keep], values[keep]))                   # by value, then root
    roots, values = roots[keep][order], values[keep][order]
    row_of_root = np.full(flat_c.size, -1, dtype=np.int32)
    row_of_root[roots] = np.arange(len(roots), dtype=np.int32)
    table = _table_host(vol, comp, row_of_root, len(roots), by_id=separate is not None)
    ids = (row_of_root[flat_c] + 1).reshape(vol.shape) if want_ids else None
    return dict(table=table, roots=roots, values=values, not_listed_objects=objects, not_listed_voxels=voxels), ids, separation


# ---- device route ----------------------------------------------------------------------------------------------------------------
def _moments_device(labels_dev, comp, row_of_root, zyx, rows: int):
    """vs_component_moments: the (rows, 20) int64 table on the device"""
    import torch
    from .. import _lib
    table = torch.empty((rows, len(FIELDS)), dtype=torch.int64, device=labels_dev.device)
    with torch.cuda.device(labels_dev.device):
        _lib.check(_lib.lib.vs_component_moments(_lib.ptr(labels_dev), _lib.ptr(comp), _lib.ptr(row_of_root), *zyx, rows, _lib.ptr(table),
                                                 _lib.stream_ptr()))
    return table


def _object_moments_device(objects, row_of_root, zyx, rows: int):
    """vs_object_moments: the (rows, 20) int64 table of a labelling by member voxel ids, on the device"""
    import torch
    from .. import _lib
    table = torch.empty((rows, len(FIELDS)), dtype=torch.int64, device=objects.device)
    with torch.cuda.device(objects.device):
        _lib.check(_lib.lib.vs_object_moments(_lib.ptr(objects), _lib.ptr(row_of_root), *zyx, rows, _lib.ptr(table), _lib.stream_ptr()))
    return table


def _measure_device(v, zyx, device, connectivity: int, min_voxels: int, background: int, include_background: bool, want_ids: bool,
                    separate: dict | None = None):
    import torch
    n = v.numel()
    lv.require_memory(device, 4 * n + (4 * n if want_ids else 0), f"the row of every root of a {tuple(zyx)} volume")
    separation = None
    if separate is None:
        comp = co.label_device(v, zyx, connectivity)
    else:
        from . import separation as sp
        comp, report, contacts = sp.separate_prepared(v, zyx, device, separate["values"], connectivity, separate["depth"], separate["max_pairs"],
                                                             separate.get("weights", lv.UNIT_WEIGHTS))
        separation = dict(report=report, contacts=contacts)
    size, _ = co.sizes_device(comp, zyx)
    roots = torch.nonzero(size).reshape(-1)                           # ascending
    sizes, values = size[roots].to(torch.int64), v[roots].to(torch.int64)
    del size
    keep = sizes >= min_voxels
    if not include_background:
        keep &= values != background
    objects = torch.zeros(256, dtype=torch.int64, device=device).index_add_(0, values[~keep], torch.ones_like(sizes[~keep]))
    voxels = torch.zeros(256, dtype=torch.int64, device=device).index_add_(0, values[~keep], sizes[~keep])
    values, order = torch.sort(values[keep], stable=True)             # by value; roots stay ascending within a value
    roots = roots[keep][order]
    rows = int(roots.numel())
    lv.require_memory(device, 8 * len(FIELDS) * rows, f"the table of {rows} components")
    row_of_root = torch.full((n,), -1, dtype=torch.int32, device=device)
    row_of_root[roots] = torch.arange(rows, dtype=torch.int32, device=device)
    table = _moments_device(v, comp, row_of_root, zyx, rows) if separate is None else _object_moments_device(comp, row_of_root, zyx, rows)
    ids = (row_of_root[comp.to(torch.int64)] + 1).cpu().numpy().reshape(zyx) if want_ids else None
    host = lambda t: t.cpu().numpy().astype(np.int64)                 # noqa: E731
    return dict(table=host(table), roots=host(roots), values=host(values), not_listed_objects=host(objects), not_listed_voxels=host(voxels)), ids, separation


# ---- public: the integers --------------------------------------------------------------------------------------------------------
def _measure(vol, connectivity, min_voxels, background, include_background, device, want_ids, separate=None):
    """``separate`` (None, or the ``values``, ``depth`` and ``max_pairs`` of ``separation.separation_settings``): measure the objects of
    ``separation.separate_objects`` in place of the components; the third result is then its report and contacts, else None"""
    _check_sums_fit(vol.shape)
    min_voxels, background = _arguments(min_voxels, background)
    shape, zyx, device, v = co.prepare(vol, connectivity, device)
    if device is None:
        raw, ids, separation = _measure_host(v, int(connectivity), min_voxels, background, bool(include_background), want_ids, separate)
    else:
        raw, ids, separation = _measure_device(v, zyx, device, int(connectivity), min_voxels, background, bool(include_background), want_ids, separate)
    raw["shape"] = np.array(zyx, dtype=np.int64)
    return raw, (None if ids is None else ids.astype(np.int32, copy=False).reshape(shape)), separation


def measure_components(vol, connectivity: int = 6, min_voxels: int = 1, background: int = 0, include_background: bool = False, device=None,
                       separate: dict | None = None) -> dict:
    """The raw integers, as int64 arrays: ``table`` (rows, 20) in the order of ``FIELDS``, ``roots`` and ``values`` (rows,),
    ``not_listed_objects`` / ``not_listed_voxels`` (256, per label value: the components that got no row) and ``shape`` (Z, Y, X).
    Row order: value ascending, then root ascending; object id = row + 1.  ``separate`` (a dict with ``values``, ``depth`` and
    ``max_pairs``, see ``utilities/separation.py``): one row per separated OBJECT - its root is the object's lowest voxel, and a face
    between two objects of one value counts as exposed."""
    return _measure(vol, connectivity, min_voxels, background, include_background, device, False, separate)[0]


def object_ids(vol, connectivity: int = 6, min_voxels: int = 1, background: int = 0, include_background: bool = False, device=None,
               separate: dict | None = None) -> np.ndarray:
    """int32 array of ``vol.shape``: the object id (row of ``measure_components`` + 1) of every voxel, 0 where it is not measured."""
    return _measure(vol, connectivity, min_voxels, background, include_background, device, True, separate)[1]


# ---- public: the derived figures ---------------------------------------------------------------------------------------------------
COLUMNS = ("id", "value", "voxels", "volume", "centroid_z", "centroid_y", "centroid_x", "min_z", "max_z", "min_y", "max_y", "min_x", "max_x",
           "extent_z", "extent_y", "extent_x", "surface_area", "equivalent_diameter", "sphericity", "axis_1", "axis_2", "axis_3", "elongation",
           "flatness", "touches_border", "root", "root_z", "root_y", "root_x")
_INT_COLUMNS = {"id", "value", "voxels", "min_z", "max_z", "min_y", "max_y", "min_x", "max_x", "extent_z", "extent_y", "extent_x", "touches_border",
                "root", "root_z", "root_y", "root_x"}


def _exact_covariance(table: np.ndarray) -> np.ndarray:
    """(rows, 3, 3) covariance of the voxel coordinates (z, y, x): the numerators n sum ab - sum a sum b in Python integers - the float
    difference cancels catastrophically for a small object far from the origin - then one division by n^2 in float64"""
    t = table.astype(object)
    n = t[:, F["voxels"]]
    first = (t[:, F["sum_z"]], t[:, F["sum_y"]], t[:, F["sum_x"]])
    second = {(0, 0): "sum_zz", (1, 1): "sum_yy", (2, 2): "sum_xx", (0, 1): "sum_zy", (0, 2): "sum_zx", (1, 2): "sum_yx"}
    cov = np.zeros((len(table), 3, 3), dtype=np.float64)
    n2 = (n * n).astype(np.float64)
    for (a, b), name in second.items():
        numerator = n * t[:, F[name]] - first[a] * first[b]
        cov[:, a, b] = cov[:, b, a] = numerator.astype(np.float64) / n2
    return cov


def object_table(raw: dict, voxel_size=1.0, shape=None) -> dict:
    """The derived figures of every object, in float64 from the integers of ``measure_components`` alone: ``{"objects": {column:
    array}, "summary": {str(value): {...}}, "voxel_size": [sz, sy, sx], "shape": [Z, Y, X]}``.

    Columns (``COLUMNS``): ``volume`` = voxels x the volume of a voxel; ``centroid_*`` in voxel coordinates; the bounding box and
    its extents in voxels; ``surface_area`` = the exposed faces across each axis x the area of a face across that axis - the
    face-count area, which OVERESTIMATES a curved surface (a sphere's by a factor of 1.5 however fine the grid);
    ``equivalent_diameter`` of the sphere of the same volume; ``sphericity`` = pi^(1/3) (6 V)^(2/3) / A with that area, so a cube scores
    0.806 and nothing scores 1; ``axis_1 >= axis_2 >= axis_3``: the square roots of the eigenvalues of the covariance matrix of the
    voxel centres in physical units (standard deviations along the principal axes); ``elongation`` = axis_2 / axis_1 and
    ``flatness`` = axis_3 / axis_2, NaN where the denominator is 0; ``touches_border``; ``root`` and its coordinates, to find the
    object in a viewer.  The summary holds per value the objects, voxels, volume, volume fraction of the whole volume, the largest
    and the median object (voxels) and the components that were not listed."""
    table = np.asarray(raw["table"], dtype=np.int64).reshape(-1, len(FIELDS))
    zyx = lv.zyx(tuple(int(s) for s in (raw["shape"] if shape is None else shape)))
    sz, sy, sx = lv.voxel_size(voxel_size)
    roots, values = np.asarray(raw["roots"], dtype=np.int64), np.asarray(raw["values"], dtype=np.int64)
    col = lambda name: table[:, F[name]]                              # noqa: E731
    n = col("voxels").astype(np.float64)
    out = {"id": np.arange(1, len(table) + 1, dtype=np.int64), "value": values, "voxels": col("voxels")}
    out["volume"] = n * (sz * sy * sx)
    with np.errstate(divide="ignore", invalid="ignore"):
        for letter in "zyx":
            out["centroid_" + letter] = col("sum_" + letter).astype(np.float64) / n
        for letter in "zyx":
            out["min_" + letter], out["max_" + letter] = col("min_" + letter), col("max_" + letter)
        for letter in "zyx":
            out["extent_" + letter] = col("max_" + letter) - col("min_" + letter) + 1
        area = col("faces_z").astype(np.float64) * (sy * sx) + col("faces_y").astype(np.float64) * (sz * sx) + col("faces_x").astype(np.float64) * (sz * sy)
        out["surface_area"] = area
        out["equivalent_diameter"] = np.cbrt(6.0 * out["volume"] / math.pi)
        out["sphericity"] = np.where(area > 0, math.pi ** (1.0 / 3.0) * np.cbrt(6.0 * out["volume"]) ** 2 / area, np.nan)
        cov = _exact_covariance(table) * np.outer((sz, sy, sx), (sz, sy, sx))
        eig = np.linalg.eigvalsh(cov)[:, ::-1] if len(table) else np.zeros((0, 3))       # descending
        axes = np.sqrt(np.clip(eig, 0.0, None))
        out["axis_1"], out["axis_2"], out["axis_3"] = axes[:, 0], axes[:, 1], axes[:, 2]
        out["elongation"] = np.where(axes[:, 0] > 0, axes[:, 1] / axes[:, 0], np.nan)
        out["flatness"] = np.where(axes[:, 1] > 0, axes[:, 2] / axes[:, 1], np.nan)
    out["touches_border"] = col("touches_border")
    out["root"] = roots
    out["root_z"], out["root_y"], out["root_x"] = (c.astype(np.int64) for c in np.unravel_index(roots, zyx))
    objects = {name: out[name] for name in COLUMNS}

    total = zyx[0] * zyx[1] * zyx[2]
    not_objects, not_voxels = np.asarray(raw["not_listed_objects"]), np.asarray(raw["not_listed_voxels"])
    summary = {}
    for value in sorted(set(values.tolist()) | set(np.flatnonzero(not_objects).tolist())):
        sizes = col("voxels")[values == value]
        voxels = int(sizes.sum())
        summary[str(int(value))] = {
            "objects": int(len(sizes)), "voxels": voxels, "volume": float(voxels * (sz * sy * sx)), "volume_fraction": voxels / total,
            "largest_object": int(sizes.max()) if len(sizes) else 0, "median_object": float(np.median(sizes)) if len(sizes) else float("nan"),
            "not_listed_objects": int(not_objects[value]), "not_listed_voxels": int(not_voxels[value])}
    return {"objects": objects, "summary": summary, "voxel_size": [sz, sy, sx], "shape": [int(s) for s in zyx]}


# ---- settings and reporting ------------------------------------------------------------------------------------------------------
def measurement_settings(settings) -> dict:
    """the optional predict-settings keys ``measure_objects``, ``measure_connectivity`` (default: ``postprocess_connectivity`` where that
    is set, else 6), ``measure_min_voxels``, ``measure_background``, ``measure_voxel_size`` (default: ``voxel_spacing`` where that is set, else
    1.0) and ``measure_save_ids`` as arguments, with ``active``: whether ``measure_objects`` asks for work"""
    connectivity = getattr(settings, "measure_connectivity", None) or getattr(settings, "postprocess_connectivity", None) or 6
    connectivity = int(connectivity)
    if connectivity not in (6, 18, 26):
        raise ValueError(f"measure_connectivity {connectivity}: it is 6, 18 or 26")
    min_voxels = getattr(settings, "measure_min_voxels", None)
    min_voxels = 1 if min_voxels is None else int(min_voxels)
    if min_voxels < 1:
        raise ValueError("measure_min_voxels must be at least 1")
    voxel_size = getattr(settings, "measure_voxel_size", None)
    grid = lv.spacing_settings(settings)
    if voxel_size is None and grid is not None:
        voxel_size = grid[0]
    return dict(active=bool(getattr(settings, "measure_objects", False)), connectivity=connectivity, min_voxels=min_voxels,
                include_background=bool(getattr(settings, "measure_background", False)),
                voxel_size=list(lv.voxel_size(1.0 if voxel_size is None else voxel_size)), save_ids=bool(getattr(settings, "measure_save_ids", False)))


def measure_label_volume(vol, settings, device=None) -> dict:
    """``measure_components`` and ``object_table`` with the settings keys: ``{"settings", "raw", "table", "ids"}`` (``ids``: the int32
    object-id volume with ``measure_save_ids``, else None).  Measures whether or not ``measure_objects`` is set: calling is the request.
    With ``measure_separate: true`` the rows and the ids are those of the separated objects (``utilities/separation.py``) and the
    result has a further key ``"separation"``: its ``settings``, the per-value ``report`` and the ``contacts`` table."""
    m = measurement_settings(settings)
    from . import separation as sp
    s = sp.separation_settings(settings)
    if not s["active"]:
        raw, ids, _ = _measure(vol, m["connectivity"], m["min_voxels"], 0, m["include_background"], device, m["save_ids"])
        return {"settings": m, "raw": raw, "table": object_table(raw, m["voxel_size"]), "ids": ids}
    raw, ids, separation = _measure(vol, m["connectivity"], m["min_voxels"], 0, m["include_background"], device, m["save_ids"], s)
    separation = dict(settings=s, report=separation["report"], contacts=sp.contacts_table(separation["contacts"], raw["roots"], m["voxel_size"], s.get("unit")))
    return {"settings": m, "raw": raw, "table": object_table(raw, m["voxel_size"]), "ids": ids, "separation": separation}


def object_table_text(table: dict, largest: int = 10) -> str:
    """the per-value summary and the ``largest`` largest objects as text, for the log"""
    lines = [f"{'value':>5} {'objects':>9} {'voxels':>12} {'volume':>14} {'fraction':>9} {'largest':>12} {'median':>10} {'not listed':>10} {'their voxels':>12}"]
    for value, row in table["summary"].items():
        lines.append(f"{value:>5} {row['objects']:>9} {row['voxels']:>12} {row['volume']:>14.6g} {row['volume_fraction']:>9.5f} "
                     f"{row['largest_object']:>12} {row['median_object']:>10.1f} {row['not_listed_objects']:>10} {row['not_listed_voxels']:>12}")
    o = table["objects"]
    order = np.lexsort((o["id"], -o["voxels"]))[:largest]
    if len(order):
        lines.append(f"the {len(order)} largest objects:")
        lines.append(f"{'id':>8} {'value':>5} {'voxels':>12} {'centroid (z, y, x)':>30} {'area':>12} {'sphericity':>10} {'elongation':>10} {'flatness':>9} {'border':>6}")
        for i in order:
            centroid = f"{o['centroid_z'][i]:.1f}, {o['centroid_y'][i]:.1f}, {o['centroid_x'][i]:.1f}"
            lines.append(f"{o['id'][i]:>8} {o['value'][i]:>5} {o['voxels'][i]:>12} {centroid:>30} {o['surface_area'][i]:>12.6g} {o['sphericity'][i]:>10.4f} "
                         f"{o['elongation'][i]:>10.4f} {o['flatness'][i]:>9.4f} {'yes' if o['touches_border'][i] else 'no':>6}")
    return "\n".join(lines)


def separation_text(m: dict) -> str:
    """what the log adds where ``measure_label_volume`` separated touching objects: the per-value report and the number of contacts;
    empty otherwise"""
    if m.get("separation") is None:
        return ""
    from . import separation as sp
    s = m["separation"]
    return (f"\nTouching objects taken apart at depth {s['settings']['depth']} ({len(s['contacts']['id_a'])} contacts):\n"
            + sp.separation_text(s["report"]))


def write_measurements(stem, raw: dict, table: dict, settings: dict | None = None, separation: dict | None = None) -> list[Path]:
    """``<stem>_objects.csv`` (one row per object, the columns of ``COLUMNS``) and ``<stem>_objects.json``: the settings, the summary
    and per object its id, value, root, the raw integers (``fields`` names them) and the derived figures - the integers make the
    file reproducible to the bit; NaN is written as null.  ``separation`` (the key of that name of ``measure_label_volume``): the rows are
    separated objects - the JSON gains a ``separation`` section (settings and per-value report) and ``<stem>_object_contacts.csv`` /
    ``.json`` are written as well."""
    stem = str(stem)
    written = [Path(stem + "_objects.csv"), Path(stem + "_objects.json")]
    o = table["objects"]
    rows = len(o["id"])

    def cell(name, i):
        return int(o[name][i]) if name in _INT_COLUMNS else float(o[name][i])

    with open(written[0], "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(COLUMNS)
        for i in range(rows):
            w.writerow([cell(name, i) if name in _INT_COLUMNS else repr(cell(name, i)) for name in COLUMNS])
    raw_table = np.asarray(raw["table"], dtype=np.int64).reshape(-1, len(FIELDS))
    doc = {"settings": settings, "shape": table["shape"], "voxel_size": table["voxel_size"], "fields": list(FIELDS),
           "summary": {value: {k: (lv.json_number(x) if isinstance(x, float) else x) for k, x in row.items()} for value, row in table["summary"].items()},
           "objects": [{"id": int(o["id"][i]), "value": int(o["value"][i]), "root": int(o["root"][i]), "raw": [int(x) for x in raw_table[i]],
                        "derived": {name: lv.json_number(o[name][i]) for name in COLUMNS if name not in _INT_COLUMNS}} for i in range(rows)]}
    if separation is not None:
        from . import separation as sp
        doc["separation"] = {"settings": sp.json_settings(separation["settings"]), "report": separation["report"]}
    with open(written[1], "w") as f:
        json.dump(doc, f, indent=1)
    if separation is not None:
        written += sp.write_contacts(stem, separation["contacts"], separation["settings"], separation["report"])
    return written


def raw_from_json(doc: dict) -> dict:
    """the raw integers back from the document ``write_measurements`` wrote (without the not-listed totals' split by object)"""
    objects = doc["objects"]
    not_objects, not_voxels = np.zeros(256, dtype=np.int64), np.zeros(256, dtype=np.int64)
    for value, row in doc["summary"].items():
        not_objects[int(value)], not_voxels[int(value)] = row["not_listed_objects"], row["not_listed_voxels"]
    return dict(table=np.array([obj["raw"] for obj in objects], dtype=np.int64).reshape(-1, len(FIELDS)),
                roots=np.array([obj["root"] for obj in objects], dtype=np.int64), values=np.array([obj["value"] for obj in objects], dtype=np.int64),
                not_listed_objects=not_objects, not_listed_voxels=not_voxels, shape=np.array(doc["shape"], dtype=np.int64))
