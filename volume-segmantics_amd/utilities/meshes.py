"""Surface meshes of a label volume: per label value the naive surface net of its voxels - a closed quad mesh one can open in a
viewer or hand to a mesher - written as binary PLY or STL.

Definitions (include/volseg_hip.h states them for the C ABI; every route gives the same bits).  ``M`` is the set of voxels of a
``Z x Y x X`` uint8 volume with value ``value``; everything outside the volume is outside ``M``, on an axis of length 1 too, so the
mesh is always closed (``measure`` counts no faces across such an axis: the two agree for extents of 2 and more).  Cell ``(k, j,
i)``, ``0 <= k <= Z``, ``0 <= j <= Y``, ``0 <= i <= X``, has the voxel centres ``(k-1 | k, j-1 | j, i-1 | i)`` as corners and the linear
index ``(k (Y+1) + j)(X+1) + i``; the cells must number fewer than 2^31.  A cell is active when its corners are neither all in ``M``
nor all outside.  There is one vertex per active cell, numbered in ascending cell index, at ``float32(base) + off`` per axis in
voxel-index coordinates ``(z, y, x)``, ``base = (k-1, j-1, i-1)``: ``off = 0.5`` for style ``blocky`` (the mesh is the voxel faces
themselves); for ``smooth`` ``off_a = float32(float64(S_a) / float64(2 n))`` over the cell's ``n`` crossing edges - the edges whose
two corners differ - with ``S_a`` the sum of twice the edge midpoints' offsets along ``a`` (the mean of the midpoints: naive surface
nets).  There is one quad per pair of face-adjacent positions of which exactly one is in ``M``: its owner is the largest-index cell
of the four around that edge; with ``(a, b, c)`` the cyclic rotation of ``(x, y, z)`` that starts at the edge's axis and offsets
``(db, dc)`` from the owner, its vertices are those of the cells ``(-1,-1), (0,-1), (0,0), (-1,0)`` when the lower position is the one
in ``M``, else ``(-1,-1), (-1,0), (0,0), (0,-1)`` - counter-clockwise seen from outside ``M`` once positions are read as right-handed
``(x, y, z)``, which is how the file writers emit them.  Quads are ordered by owner cell index, then axis z, y, x; quad ``(v0, v1,
v2, v3)`` splits into the triangles ``(v0, v1, v2)`` and ``(v0, v2, v3)``.  Where two voxels of ``M`` touch only along an edge that
edge carries 4 quads: the non-manifold edge is kept.  The quads across an axis number exactly the exposed faces across it.

Routes: ``vs_mesh_count`` / ``vs_mesh_emit`` (csrc/mesh.hip) on a GPU; shifted comparisons on a padded mask, ``flatnonzero`` and
``cumsum`` on a host.  ``mesh_summary`` works in float64 from the arrays alone, by the same code, so its figures agree bit for bit.

Not here: smoothing or relaxation iterations, decimation, per-object meshes, surfaces shared between materials, marching cubes."""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np

from . import label_volume as lv

STYLES = {"smooth": 0, "blocky": 1}            # include/volseg_hip.h VS_MESH_SMOOTH / VS_MESH_BLOCKY
FORMATS = ("ply", "stl")
CELL_LIMIT = 1 << 31
AXES = ("z", "y", "x")


# ---- arguments -------------------------------------------------------------------------------------------------------------------
def _check(shape, value, style) -> tuple[tuple[int, int, int], int, str]:
    zyx = lv.zyx(shape)
    cells = (zyx[0] + 1) * (zyx[1] + 1) * (zyx[2] + 1)
    if cells >= CELL_LIMIT:
        raise ValueError(f"a volume of shape {tuple(shape)} has {cells} cells: a mesh needs fewer than 2^31 (vertex ids are int32)")
    value = int(value)
    if not 0 <= value <= 255:
        raise ValueError(f"value {value} is not a uint8 value")
    if style not in STYLES:
        raise ValueError(f"mesh style {style!r}: it is one of {sorted(STYLES)}")
    return zyx, value, style


def _check_counts(vertices: int, quads_per_axis) -> None:
    if vertices >= CELL_LIMIT or sum(int(q) for q in quads_per_axis) >= CELL_LIMIT:
        raise ValueError(f"{vertices} vertices and {sum(int(q) for q in quads_per_axis)} quads: each must stay below 2^31")


def smooth_offsets() -> np.ndarray:
    """(256, 3) float32: ``off`` (z, y, x) of style ``smooth`` per corner mask, bit ``4 dz + 2 dy + dx``; 0.5 for the two masks that are not active"""
    table = np.full((256, 3), 0.5, dtype=np.float32)
    weight = (4, 2, 1)
    for mask in range(1, 255):
        s, n = [0, 0, 0], 0
        for a in range(3):
            b, c = (a + 1) % 3, (a + 2) % 3
            for u in (0, 1):
                for v in (0, 1):
                    lo = u * weight[b] + v * weight[c]
                    if ((mask >> lo) ^ (mask >> (lo + weight[a]))) & 1:
                        n += 1
                        s[a] += 1
                        s[b] += 2 * u
                        s[c] += 2 * v
        table[mask] = (np.array(s, dtype=np.float64) / np.float64(2 * n)).astype(np.float32)
    return table


# ---- host route ------------------------------------------------------------------------------------------------------------------
def _surface_host(vol: np.ndarray, value: int, style: str):
    z, y, x = vol.shape
    inside = np.zeros((z + 2, y + 2, x + 2), dtype=bool)
    inside[1:-1, 1:-1, 1:-1] = vol == value
    corner = lambda dz, dy, dx: inside[dz:dz + z + 1, dy:dy + y + 1, dx:dx + x + 1]      # noqa: E731  of every cell (k, j, i)
    code = np.zeros((z + 1, y + 1, x + 1), dtype=np.uint8)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                code |= corner(dz, dy, dx).astype(np.uint8) << np.uint8(4 * dz + 2 * dy + dx)
    code = code.reshape(-1)
    active = (code != 0) & (code != 255)
    cells = np.flatnonzero(active)                                    # ascending cell index: the vertex order
    ids = np.cumsum(active, dtype=np.int32)
    ids -= 1                                                          # the vertex id at every active cell
    k, j, i = np.unravel_index(cells, (z + 1, y + 1, x + 1))
    off = smooth_offsets()[code[cells]] if style == "smooth" else np.full((len(cells), 3), 0.5, dtype=np.float32)
    vertices = np.stack([(c - 1).astype(np.float32) for c in (k, j, i)], axis=1) + off

    first = corner(0, 0, 0).reshape(-1)
    owned = np.stack([first ^ corner(1, 0, 0).reshape(-1), first ^ corner(0, 1, 0).reshape(-1), first ^ corner(0, 0, 1).reshape(-1)], axis=1)
    per_axis = owned.sum(axis=0, dtype=np.int64)
    hits = np.flatnonzero(owned.reshape(-1))                          # owner x 3 + axis, ascending: the quad order
    owner, axis = hits // 3, hits % 3
    sk, sj = (y + 1) * (x + 1), x + 1
    back = np.array([[-sj - 1, -sj, -1], [-sk - 1, -1, -sk], [-sk - sj, -sk, -sj]], dtype=np.int64)     # per axis: v0, then v1 and v3 when the lower one is in M
    lower = first[owner]
    one, other = ids[owner + back[axis, 1]], ids[owner + back[axis, 2]]
    quads = np.stack([ids[owner + back[axis, 0]], np.where(lower, one, other), ids[owner], np.where(lower, other, one)], axis=1).astype(np.int32)
    return vertices.astype(np.float32).reshape(-1, 3), quads.reshape(-1, 4), per_axis


# ---- device route ----------------------------------------------------------------------------------------------------------------
def _surface_device(labels_dev, zyx, value: int, style: str):
    import torch
    from .. import _lib
    device = labels_dev.device
    need = int(_lib.lib.vs_mesh_workspace_bytes(*zyx))
    lv.require_memory(device, need + 32, f"the mesh workspace of a {tuple(zyx)} volume")
    work = torch.empty(need, dtype=torch.uint8, device=device)
    totals = torch.empty(4, dtype=torch.int64, device=device)
    with torch.cuda.device(device):
        _lib.check(_lib.lib.vs_mesh_count(_lib.ptr(labels_dev), *zyx, value, _lib.ptr(work), need, _lib.ptr(totals), _lib.stream_ptr()))
        counts = [int(t) for t in totals.cpu()]
        n_vertices, n_quads = counts[0], sum(counts[1:])
        _check_counts(n_vertices, counts[1:])
        lv.require_memory(device, 12 * n_vertices + 16 * n_quads, f"the {n_vertices} vertices and {n_quads} quads of value {value}")
        vertices = torch.empty((n_vertices, 3), dtype=torch.float32, device=device)
        quads = torch.empty((n_quads, 4), dtype=torch.int32, device=device)
        if n_vertices or n_quads:
            _lib.check(_lib.lib.vs_mesh_emit(_lib.ptr(labels_dev), *zyx, value, STYLES[style], _lib.ptr(work), need, _lib.ptr(vertices), _lib.ptr(quads),
                                             _lib.stream_ptr()))
    return vertices.cpu().numpy(), quads.cpu().numpy(), np.array(counts[1:], dtype=np.int64)


# ---- public: the arrays ------------------------------------------------------------------------------------------------------------
def _labels(vol, device):
    """(device or None, the volume as a host (Z, Y, X) array or a flat aligned device tensor); the upload is all the memory asked for here"""
    _, _, device, v = lv.prepare(vol, device, lambda zyx, resident: 0 if resident else int(np.prod(zyx)), "labels")
    return device, v


def _extract(v, zyx, device, value: int, style: str) -> dict:
    if device is None:
        vertices, quads, per_axis = _surface_host(v, value, style)
        _check_counts(len(vertices), per_axis)
    else:
        vertices, quads, per_axis = _surface_device(v, zyx, value, style)
    return dict(vertices=vertices, quads=quads, quads_per_axis=per_axis, shape=np.array(zyx, dtype=np.int64))


def extract_surface(vol, value, style: str = "smooth", device=None) -> dict:
    """The surface of the voxels of ``vol`` with value ``value``: ``vertices`` (V, 3) float32 in voxel-index coordinates (z, y, x),
    ``quads`` (Q, 4) int32 vertex ids, ``quads_per_axis`` (3,) int64 - the quads across z, y and x - and ``shape`` (Z, Y, X).  The HIP
    kernels where ``device`` (default: the volume's, else the current GPU) is one, the host route otherwise: the same bits."""
    zyx, value, style = _check(tuple(vol.shape), value, style)
    device, v = _labels(vol, device)
    return _extract(v, zyx, device, value, style)


# ---- public: the figures -----------------------------------------------------------------------------------------------------------
def _positions_xyz(vertices, voxel_size) -> np.ndarray:
    """(V, 3) float64 right-handed (x, y, z) in physical units"""
    sz, sy, sx = lv.voxel_size(voxel_size)
    p = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    return np.stack([p[:, 2] * sx, p[:, 1] * sy, p[:, 0] * sz], axis=1)


def triangles_of(quads) -> np.ndarray:
    """(2 Q, 3): per quad (v0, v1, v2) then (v0, v2, v3)"""
    q = np.asarray(quads).reshape(-1, 4)
    return np.stack([q[:, [0, 1, 2]], q[:, [0, 2, 3]]], axis=1).reshape(-1, 3)


def mesh_summary(surface: dict, voxel_size=1.0) -> dict:
    """Figures of one mesh, in float64 from the arrays alone: ``vertices``, ``quads_z / _y / _x``, ``quads``, ``triangles``;
    ``surface_area`` (the sum of the triangle areas) and ``enclosed_volume`` (divergence theorem over the triangles: positive for the
    outward winding) in physical units; ``closed`` (every directed edge u -> v occurs as often as v -> u); ``edges`` (distinct undirected
    quad edges) and ``euler_characteristic`` = V - E + F over the quads; ``non_manifold_edges`` (edges with more than 2 quads);
    ``bounding_box`` [[z, y, x] min, [z, y, x] max] in physical units, None for an empty mesh."""
    quads = np.asarray(surface["quads"], dtype=np.int64).reshape(-1, 4)
    per_axis = [int(q) for q in surface["quads_per_axis"]]
    sz, sy, sx = lv.voxel_size(voxel_size)
    p = _positions_xyz(surface["vertices"], (sz, sy, sx))
    n_vertices = len(p)
    tri = triangles_of(quads)
    a, b, c = p[tri[:, 0]], p[tri[:, 1]], p[tri[:, 2]]
    cross = np.cross(b - a, c - a) if len(tri) else np.zeros((0, 3))
    area = float(np.sqrt((cross * cross).sum(axis=1)).sum() / 2.0)
    volume = float((a * np.cross(b, c)).sum() / 6.0) if len(tri) else 0.0
    start, end = quads.reshape(-1), quads[:, [1, 2, 3, 0]].reshape(-1)
    forward, backward = np.sort(start * n_vertices + end), np.sort(end * n_vertices + start)
    undirected, uses = np.unique(np.minimum(start, end) * n_vertices + np.maximum(start, end), return_counts=True)
    box = None if n_vertices == 0 else [[float(p[:, 2].min()), float(p[:, 1].min()), float(p[:, 0].min())],
                                        [float(p[:, 2].max()), float(p[:, 1].max()), float(p[:, 0].max())]]
    return {"vertices": n_vertices, "quads_z": per_axis[0], "quads_y": per_axis[1], "quads_x": per_axis[2], "quads": len(quads),
            "triangles": 2 * len(quads), "surface_area": area, "enclosed_volume": volume, "closed": bool(np.array_equal(forward, backward)),
            "edges": int(len(undirected)), "euler_characteristic": int(n_vertices - len(undirected) + len(quads)),
            "non_manifold_edges": int((uses > 2).sum()), "bounding_box": box}


# ---- public: the files -------------------------------------------------------------------------------------------------------------
def _file_positions(vertices, voxel_size) -> np.ndarray:
    """(x, y, z) = (p_x s_x, p_y s_y, p_z s_z), computed in float64 and stored as float32"""
    return _positions_xyz(vertices, voxel_size).astype("<f4")


def write_ply(path, surface: dict, voxel_size=1.0, triangulate: bool = False) -> Path:
    """binary little-endian PLY: vertices as float x, y, z; faces as ``list uchar int`` - the quads, or with ``triangulate`` their triangles"""
    path = Path(path)
    p = _file_positions(surface["vertices"], voxel_size)
    faces = triangles_of(surface["quads"]) if triangulate else np.asarray(surface["quads"]).reshape(-1, 4)
    corners = faces.shape[1]
    records = np.empty(len(faces), dtype=[("n", "u1"), ("v", "<i4", (corners,))])
    records["n"], records["v"] = corners, faces
    header = ("ply\nformat binary_little_endian 1.0\ncomment volume_segmantics_amd surface net\n"
              f"element vertex {len(p)}\nproperty float x\nproperty float y\nproperty float z\n"
              f"element face {len(faces)}\nproperty list uchar int vertex_indices\nend_header\n")
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(p.tobytes())
        f.write(records.tobytes())
    return path


def write_stl(path, surface: dict, voxel_size=1.0) -> Path:
    """binary STL: an 80-byte header, the triangle count, per triangle the unit normal from the winding (0 for a triangle without area),
    its three corners and a zero attribute word"""
    path = Path(path)
    p = _positions_xyz(surface["vertices"], voxel_size)
    tri = triangles_of(surface["quads"])
    a, b, c = p[tri[:, 0]], p[tri[:, 1]], p[tri[:, 2]]
    normal = np.cross(b - a, c - a) if len(tri) else np.zeros((0, 3))
    length = np.sqrt((normal * normal).sum(axis=1, keepdims=True))
    normal = np.divide(normal, length, out=np.zeros_like(normal), where=length > 0)
    records = np.zeros(len(tri), dtype=[("normal", "<f4", (3,)), ("a", "<f4", (3,)), ("b", "<f4", (3,)), ("c", "<f4", (3,)), ("attribute", "<u2")])
    records["normal"], records["a"], records["b"], records["c"] = normal, a, b, c
    with open(path, "wb") as f:
        f.write(b"volume_segmantics_amd surface net".ljust(80, b" "))
        f.write(np.array(len(tri), dtype="<u4").tobytes())
        f.write(records.tobytes())
    return path


# ---- settings and reporting ------------------------------------------------------------------------------------------------------
def mesh_settings(settings) -> dict:
    """the optional predict-settings keys ``mesh_surfaces``, ``mesh_values`` (a list; default None: every non-zero value present),
    ``mesh_style`` (smooth | blocky), ``mesh_format`` (ply | stl), ``mesh_triangulate`` and ``mesh_voxel_size`` (one number or [sz, sy,
    sx]; default ``measure_voxel_size`` where that is set, else ``voxel_spacing``, else 1.0) as arguments, with ``active``: whether ``mesh_surfaces`` asks for work"""
    style = getattr(settings, "mesh_style", None) or "smooth"
    if style not in STYLES:
        raise ValueError(f"mesh_style {style!r}: it is one of {sorted(STYLES)}")
    fmt = getattr(settings, "mesh_format", None) or "ply"
    if fmt not in FORMATS:
        raise ValueError(f"mesh_format {fmt!r}: it is one of {list(FORMATS)}")
    values = getattr(settings, "mesh_values", None)
    if values is not None:
        values = sorted({int(v) for v in (values if isinstance(values, (list, tuple)) else [values])})
        if any(not 0 <= v <= 255 for v in values):
            raise ValueError(f"mesh_values {values}: every one is a uint8 value")
    voxel_size = getattr(settings, "mesh_voxel_size", None)
    if voxel_size is None:
        voxel_size = getattr(settings, "measure_voxel_size", None)
    grid = lv.spacing_settings(settings)
    if voxel_size is None and grid is not None:
        voxel_size = grid[0]
    return dict(active=bool(getattr(settings, "mesh_surfaces", False)), values=values, style=style, format=fmt,
                triangulate=bool(getattr(settings, "mesh_triangulate", False)), voxel_size=list(lv.voxel_size(1.0 if voxel_size is None else voxel_size)))


def mesh_label_volume(vol, settings, device=None) -> dict:
    """``extract_surface`` and ``mesh_summary`` per value with the settings keys: ``{"settings", "surfaces": {value: surface}, "summary":
    {str(value): figures}, "shape"}``.  Meshes whether or not ``mesh_surfaces`` is set: calling is the request."""
    m = mesh_settings(settings)
    zyx, _, _ = _check(tuple(vol.shape), 0, m["style"])
    device, v = _labels(vol, device)
    values = m["values"]
    if values is None:
        present = np.flatnonzero(np.bincount(v.reshape(-1), minlength=256)) if device is None else np.flatnonzero(_bincount_device(v))
        values = [int(c) for c in present if c != 0]
    surfaces = {value: _extract(v, zyx, device, value, m["style"]) for value in values}
    summary = {str(value): mesh_summary(s, m["voxel_size"]) for value, s in surfaces.items()}
    return {"settings": m, "surfaces": surfaces, "summary": summary, "shape": [int(s) for s in zyx]}


def _bincount_device(v) -> np.ndarray:
    """256 counts: which values occur"""
    import torch
    lv.require_memory(v.device, 8 * 256, "the histogram of the label values")
    return torch.bincount(v, minlength=256).cpu().numpy()


def mesh_summary_text(summary: dict) -> str:
    """the per-value figures as text, for the log"""
    lines = [f"{'value':>5} {'vertices':>11} {'quads z':>10} {'quads y':>10} {'quads x':>10} {'triangles':>11} {'area':>14} {'volume':>14} {'closed':>6} {'euler':>7}"]
    for value, row in summary.items():
        lines.append(f"{value:>5} {row['vertices']:>11} {row['quads_z']:>10} {row['quads_y']:>10} {row['quads_x']:>10} {row['triangles']:>11} "
                     f"{row['surface_area']:>14.6g} {row['enclosed_volume']:>14.6g} {'yes' if row['closed'] else 'no':>6} {row['euler_characteristic']:>7}")
    return "\n".join(lines)


def write_meshes(stem, meshes: dict) -> list[Path]:
    """per value ``<stem>_mesh_<value>.<ext>`` (``mesh_format``; PLY holds quads unless ``mesh_triangulate``) and ``<stem>_meshes.json``: the
    settings, the shape and the summary per value with the file's name"""
    stem, m = str(stem), meshes["settings"]
    written, doc = [], {"settings": m, "shape": meshes["shape"], "meshes": {}}
    for value, surface in meshes["surfaces"].items():
        path = Path(f"{stem}_mesh_{value}.{m['format']}")
        if m["format"] == "ply":
            write_ply(path, surface, m["voxel_size"], m["triangulate"])
        else:
            write_stl(path, surface, m["voxel_size"])
        written.append(path)
        doc["meshes"][str(value)] = dict(meshes["summary"][str(value)], file=path.name)
    written.append(Path(stem + "_meshes.json"))
    with open(written[-1], "w") as f:
        json.dump(doc, f, indent=1)
    return written
