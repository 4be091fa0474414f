"""What the connected-component tests share (tests/test_components_host.py, tests/test_hip_components.py): oracles that use neither
route of utilities/components.py - a plain flood fill over an explicit neighbour list, scipy.ndimage.label per value with the roots
made canonical by np.minimum.at where scipy imports, a per-component restatement of the cleanup rules in plain Python - and the
volumes the tests label.  Every volume is built once and never written to."""
import functools
import itertools
import json
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden"
CONNECTIVITIES = (6, 18, 26)
RANK = {6: 1, 18: 2, 26: 3}


def neighbour_offsets(connectivity):
    """all 6 / 18 / 26 offsets (dz, dy, dx)"""
    return [d for d in itertools.product((-1, 0, 1), repeat=3) if 0 < sum(c != 0 for c in d) <= RANK[connectivity]]


def flood_roots(vol, connectivity):
    """int32 roots by flood fill: voxels in index order, each unvisited one starts a component and is its root"""
    vol = np.asarray(vol)
    z, y, x = vol.shape
    padded = np.full((z + 2, y + 2, x + 2), -1, dtype=np.int64)
    padded[1:-1, 1:-1, 1:-1] = vol
    flat = padded.reshape(-1).tolist()
    sy, sz = x + 2, (x + 2) * (y + 2)
    # an axis of length 1 has no neighbours: the padding sees to that
    deltas = [dz * sz + dy * sy + dx for dz, dy, dx in neighbour_offsets(connectivity)]
    root = [-1] * len(flat)
    inner = (np.arange(z)[:, None, None] + 1) * sz + (np.arange(y)[None, :, None] + 1) * sy + np.arange(x)[None, None, :] + 1
    order = inner.reshape(-1).tolist()
    to_linear = {p: i for i, p in enumerate(order)}
    for start in order:
        if root[start] >= 0:
            continue
        value, mark = flat[start], to_linear[start]
        root[start] = mark
        stack = [start]
        while stack:
            p = stack.pop()
            for d in deltas:
                q = p + d
                if flat[q] == value and root[q] < 0:
                    root[q] = mark
                    stack.append(q)
    return np.array([root[p] for p in order], dtype=np.int32).reshape(vol.shape)


def scipy_roots(vol, connectivity):
    """the same from scipy.ndimage.label per value, or None where scipy does not import"""
    try:
        from scipy import ndimage
    except ImportError:
        return None
    vol = np.asarray(vol)
    structure = ndimage.generate_binary_structure(3, RANK[connectivity])
    out = np.empty(vol.size, dtype=np.int64)
    index = np.arange(vol.size)
    for value in np.unique(vol):
        labelled, count = ndimage.label(vol == value, structure=structure)
        flat = labelled.reshape(-1)
        lowest = np.full(count + 1, vol.size, dtype=np.int64)
        np.minimum.at(lowest, flat, index)
        out[flat != 0] = lowest[flat[flat != 0]]
    return out.astype(np.int32).reshape(vol.shape)


def oracle_roots(vol, connectivity):
    """scipy where it imports (checked against the flood fill on the small volumes by the host tests), the flood fill otherwise"""
    got = scipy_roots(vol, connectivity)
    return flood_roots(vol, connectivity) if got is None else got


def oracle_sizes(vol, roots):
    """(size, touches) as vs_component_sizes writes them"""
    vol, flat = np.asarray(vol), np.asarray(roots).reshape(-1)
    size = np.bincount(flat, minlength=flat.size).astype(np.int32)
    touches = np.zeros(flat.size, dtype=np.uint8)
    coords = np.indices(vol.shape).reshape(3, -1)
    for axis in range(3):
        if vol.shape[axis] > 1:
            touches[flat[(coords[axis] == 0) | (coords[axis] == vol.shape[axis] - 1)]] = 1
    return size, touches


def oracle_largest(vol, roots):
    """256 roots: the largest component per value, the lower root on a tie, -1 where the value does not occur"""
    flat_v, flat_r = np.asarray(vol).reshape(-1), np.asarray(roots).reshape(-1)
    best = {}
    for r, count in zip(*np.unique(flat_r, return_counts=True)):
        c = int(flat_v[r])
        if c not in best or count > best[c][0]:             # roots ascend: a tie keeps the earlier one
            best[c] = (int(count), int(r))
    return np.array([best[c][1] if c in best else -1 for c in range(256)], dtype=np.int64)


def oracle_clean(vol, connectivity, min_size=None, keep_largest=None, hole_max=0, background=0, roots=None):
    """(cleaned volume, [components cleared, voxels cleared, holes filled, voxels filled], per-value rows) - component by component.
    min_size: {value: size}; keep_largest: set of values"""
    vol = np.asarray(vol)
    min_size, keep_largest = dict(min_size or {}), set(keep_largest or ())
    roots = oracle_roots(vol, connectivity) if roots is None else np.asarray(roots)
    flat_v, flat_r = vol.reshape(-1), roots.reshape(-1)
    size, touches = {}, {}
    coords = np.indices(vol.shape).reshape(3, -1)
    on_face = np.zeros(flat_v.size, dtype=bool)
    for a in range(3):
        if vol.shape[a] > 1:
            on_face |= (coords[a] == 0) | (coords[a] == vol.shape[a] - 1)
    uniq, counts = np.unique(flat_r, return_counts=True)
    size = dict(zip(uniq.tolist(), counts.tolist()))
    touches = set(np.unique(flat_r[on_face]).tolist())
    largest = oracle_largest(vol, roots)

    def is_cleared(r):
        c = int(flat_v[r])
        if c == background:
            return False
        return size[r] < min_size.get(c, 0) or (c in keep_largest and r != largest[c])

    final = {}
    totals = [0, 0, 0, 0]
    rows = {}
    for r in uniq.tolist():
        c = int(flat_v[r])
        row = rows.setdefault(str(c), dict(components=0, voxels=0, components_cleared=0, voxels_cleared=0, components_kept=0, voxels_kept=0))
        row["components"] += 1
        row["voxels"] += size[r]
        final[r] = c
        if is_cleared(r):
            final[r] = background
            totals[0] += 1
            totals[1] += size[r]
            row["components_cleared"] += 1
            row["voxels_cleared"] += size[r]
        else:
            row["components_kept"] += 1
            row["voxels_kept"] += size[r]
        if c == background and hole_max > 0 and size[r] <= hole_max and r not in touches and r > 0:
            front = r - 1
            value = background if is_cleared(int(flat_r[front])) else int(flat_v[front])
            if value != background:
                final[r] = value
                totals[2] += 1
                totals[3] += size[r]
    lut = np.zeros(flat_v.size, dtype=np.uint8)
    for r, value in final.items():
        lut[r] = value
    return lut[flat_r].reshape(vol.shape), totals, rows


# ---- volumes ---------------------------------------------------------------------------------------------------------------------
def random_labels(shape, k, density, seed):
    """values 0..k-1: 0 with probability 1 - density, the others share the rest"""
    rng = np.random.default_rng(seed)
    v = np.where(rng.random(shape) < density, rng.integers(1, max(k, 2), shape), 0) if k > 2 else (rng.random(shape) < density)
    return np.ascontiguousarray(v).astype(np.uint8)


def snake_rows(shape=(9, 40, 130)):
    """a one-voxel-wide serpentine of value 1 in a volume of 0 that winds through every row: along a row, one or two voxels over to a
    later row at alternating ends, along that row the other way, .. to the far corner of the plane; one voxel joins a plane to the
    plane after next, at alternating ends of the plane's path.  One component whose root is voxel 0 and whose far end is voxel n - 1
    (an odd number of full rows per plane and of full planes sees to that)"""
    z, y, x = shape
    assert z % 2 == 1 and y >= 3
    full = (y + 1) // 2
    full -= 1 - full % 2                                     # rows the path runs along: an odd count
    gaps = [1] * (full - 1)
    for i in range(y - (2 * full - 1)):                      # the rows left over: some steps between rows are two voxels long
        gaps[i] += 1
    plane = np.zeros((y, x), dtype=np.uint8)
    row, at = 0, 0
    for k in range(full):
        plane[row, :] = 1
        at = x - 1 - at
        if k < full - 1:
            for _ in range(gaps[k]):
                row += 1
                plane[row, at] = 1
            row += 1
    assert row == y - 1 and at == x - 1
    vol = np.zeros(shape, dtype=np.uint8)
    vol[0::2] = plane
    for j, zi in enumerate(range(1, z, 2)):
        vol[(zi, y - 1, x - 1) if j % 2 == 0 else (zi, 0, 0)] = 1
    return vol


def checkerboard(shape=(9, 10, 70)):
    zi, yi, xi = np.indices(shape)
    return ((zi + yi + xi) % 2).astype(np.uint8)


def shells(shape=(19, 21, 135)):
    """concentric box shells of alternating values around the centre, one voxel thick: they cross every tile boundary"""
    zi, yi, xi = np.indices(shape)
    depth = np.minimum.reduce([zi, shape[0] - 1 - zi, yi, shape[1] - 1 - yi, xi, shape[2] - 1 - xi])
    return (1 + depth % 3).astype(np.uint8)


def pair_touching(kind, at, shape=(18, 18, 132)):
    """two voxels of value 1 in a volume of 0 that touch only by an edge (kind 'edge') or only by a corner ('corner'); the second voxel
    is `at` = (z, y, x), the first one sits one step back on two / three axes - so `at` = a multiple of the tile extents puts the pair
    across a tile face, edge or corner"""
    vol = np.zeros(shape, dtype=np.uint8)
    z, y, x = at
    vol[z, y, x] = 1
    if kind == "edge_yx":
        vol[z, y - 1, x - 1] = 1
    elif kind == "edge_zx":
        vol[z - 1, y, x - 1] = 1
    elif kind == "edge_zy":
        vol[z - 1, y - 1, x] = 1
    elif kind == "edge_zy_up":
        vol[z - 1, y + 1, x] = 1
    elif kind == "edge_yx_up":
        vol[z, y - 1, x + 1] = 1
    elif kind == "corner":
        vol[z - 1, y - 1, x - 1] = 1
    elif kind == "corner_up":
        vol[z - 1, y + 1, x + 1] = 1
    else:
        raise ValueError(kind)
    return vol


PAIR_KINDS = {"edge_yx": 18, "edge_zx": 18, "edge_zy": 18, "edge_zy_up": 18, "edge_yx_up": 18, "corner": 26, "corner_up": 26}   # the least connectivity that joins


def cleanup_scene():
    """(40, 48, 72), values 0 .. 3: what the cleanup tests need in one volume (sizes in SCENE).
     * a big object of value 1 with hole A of 5 voxels inside it (the voxel in front of its root is of value 1), and with a bar of
       value 2 (4 voxels) followed by hole B of 3 voxels: B borders both values and the voxel in front of its root is the bar;
     * two more objects of value 2 of equal size 27: the tie the lower root wins;
     * an object of value 3 (26 voxels) around a 1-voxel hole C: cleared, its hole stays background;
     * a second object of value 1 against the x = 71 face with a background pocket of 4 voxels that is open to that face: never filled."""
    vol = np.zeros((40, 48, 72), dtype=np.uint8)
    vol[4:20, 4:30, 4:60] = 1
    vol[8, 8, 10:15] = 0
    vol[12, 12, 20:24] = 2
    vol[12, 12, 24:27] = 0
    vol[25:28, 5:8, 5:8] = 2
    vol[25:28, 5:8, 40:43] = 2
    vol[32:35, 10:13, 10:13] = 3
    vol[33, 11, 11] = 0
    vol[30:36, 0:6, 60:72] = 1
    vol[32:34, 2:4, 71] = 0
    vol.setflags(write=False)
    return vol


SCENE = dict(hole_a=5, hole_b=3, hole_c=1, bar=4, twin=27, object_3=26, pocket=4)


@functools.lru_cache(maxsize=None)
def vessels():
    """the committed 256^3 fixture (values 0 and 255), read-only"""
    from volume_segmantics_amd.utilities import base_data_utils as U
    vol = np.ascontiguousarray(U.numpy_from_hdf5(GOLDEN / "vessels_256cube_LABELS.h5", "/data")[0])
    vol.setflags(write=False)
    return vol


@functools.lru_cache(maxsize=None)
def vessels_expected():
    return json.loads((GOLDEN / "components_vessels.json").read_text())


VESSELS_CLEANUPS = {"keep_largest": dict(keep_largest=True), "min_object_size_80000": dict(min_object_size=80000), "fill_holes_600": dict(fill_holes=600)}
