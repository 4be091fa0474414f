"""What the separation tests share, and neither route of utilities/separation.py: a brute-force oracle written from the definitions
with plain per-voxel loops and dicts, the named scenes and the committed figures of a crop of the vessels fixture.

Oracle.  R is thickness_cases.exact_r (three exact min-plus passes).  The key of a voxel is the Python integer (R << 32) | (0xFFFFFFFF
- index); the parent of a voxel is the holder of the largest key among itself and its neighbours, a basin is where the chain of
parents ends, the pair table is a dict over every adjacent voxel pair, the merge is a dict union-find over the sorted rows and an
object is the lowest voxel of a merged set.  Nothing is vectorised and nothing is shared with the code under test."""
import functools
import json
import math
from pathlib import Path

import numpy as np

import components_cases as cc
import thickness_cases as tc

GOLDEN_VESSELS = cc.GOLDEN / "separation_vessels.json"
DEPTHS = (0.0, 1.0, 2.0)


# ---- the oracle --------------------------------------------------------------------------------------------------------------------
def offsets(connectivity):
    rank = cc.RANK[connectivity]
    return [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
            if (dz, dy, dx) != (0, 0, 0) and (dz != 0) + (dy != 0) + (dx != 0) <= rank]


def distance_map(vol, value):
    """int64 (Z, Y, X): R of `value`, 0 off it; None when the volume holds no other value (or not the value at all)"""
    vol = np.asarray(vol)
    if not (vol == value).any():
        return None
    return tc.exact_r(vol, value)


def oracle_parents(r, connectivity):
    """flat int32: the parent of every voxel with r > 0, -1 elsewhere"""
    big_z, big_y, big_x = r.shape
    offs = offsets(connectivity)
    parent = np.full(r.size, -1, dtype=np.int32)
    rl = r.tolist()
    for z in range(big_z):
        for y in range(big_y):
            for x in range(big_x):
                rv = rl[z][y][x]
                if rv == 0:
                    continue
                v = (z * big_y + y) * big_x + x
                best_key, best = (rv << 32) | (0xFFFFFFFF - v), v
                for dz, dy, dx in offs:
                    zz, yy, xx = z + dz, y + dy, x + dx
                    if 0 <= zz < big_z and 0 <= yy < big_y and 0 <= xx < big_x and rl[zz][yy][xx] > 0:
                        u = (zz * big_y + yy) * big_x + xx
                        key = (rl[zz][yy][xx] << 32) | (0xFFFFFFFF - u)
                        if key > best_key:
                            best_key, best = key, u
                parent[v] = best
    return parent


def oracle_basins(parent):
    """flat int32: the peak at which every voxel's chain ends, -1 where there is no parent"""
    basin = np.full(parent.size, -1, dtype=np.int32)
    p = parent.tolist()
    known = {}
    for v in range(len(p)):
        if p[v] < 0:
            continue
        chain, u = [], v
        while u not in known and p[u] != u:
            chain.append(u)
            u = p[u]
        peak = known.get(u, u)
        for w in chain:
            known[w] = peak
        known[u] = peak
        basin[v] = peak
    return basin


def oracle_pairs(r, basin, connectivity):
    """({(A, B): [saddle, faces_z, faces_y, faces_x]} over the adjacent basins A < B, the adjacent voxel pairs in different basins)"""
    big_z, big_y, big_x = r.shape
    offs = [o for o in offsets(connectivity) if o < (0, 0, 0)]          # every pair at its later voxel
    rl, b = r.tolist(), basin.tolist()
    rows, count = {}, 0
    for z in range(big_z):
        for y in range(big_y):
            for x in range(big_x):
                v = (z * big_y + y) * big_x + x
                if b[v] < 0:
                    continue
                for dz, dy, dx in offs:
                    zz, yy, xx = z + dz, y + dy, x + dx
                    if not (0 <= zz < big_z and 0 <= yy < big_y and 0 <= xx < big_x):
                        continue
                    u = (zz * big_y + yy) * big_x + xx
                    if b[u] < 0 or b[u] == b[v]:
                        continue
                    count += 1
                    row = rows.setdefault((min(b[u], b[v]), max(b[u], b[v])), [0, 0, 0, 0])
                    row[0] = max(row[0], min(rl[z][y][x], rl[zz][yy][xx]))
                    if (dz != 0) + (dy != 0) + (dx != 0) == 1:
                        row[1 + (0 if dz else 1 if dy else 2)] += 1
    return rows, count


def oracle_merge(rows, peak_r, depth):
    """({peak: the lowest peak of its merged set}, merges): union-find over the rows by (saddle descending, A, B)"""
    link = {p: p for p in peak_r}
    height = dict(peak_r)

    def find(p):
        while link[p] != p:
            p = link[p]
        return p

    merges = 0
    for (a, b), row in sorted(rows.items(), key=lambda item: (-item[1][0], item[0][0], item[0][1])):
        fa, fb = find(a), find(b)
        if fa != fb and math.sqrt(float(min(height[fa], height[fb]))) - math.sqrt(float(row[0])) < depth:
            lo, hi = min(fa, fb), max(fa, fb)
            link[hi] = lo
            height[lo] = max(height[fa], height[fb])
            merges += 1
    return {p: find(p) for p in link}, merges


def oracle_value(vol, value, connectivity):
    """the stages of one value that do not depend on the depth: dict(r, parent, basin, rows, count, peak_r), or None where the value is
    absent or fills the volume"""
    r = distance_map(vol, value)
    if r is None:
        return None
    parent = oracle_parents(r, connectivity)
    basin = oracle_basins(parent)
    rows, count = oracle_pairs(r, basin, connectivity)
    flat_r = r.reshape(-1)
    peaks = np.flatnonzero(basin == np.arange(basin.size))
    return dict(r=r, parent=parent, basin=basin, rows=rows, count=count, peak_r={int(p): int(flat_r[p]) for p in peaks})


def oracle_separate(vol, connectivity, depth, values=None, stages=None):
    """(objects flat int32, {value: report}, {(object a, object b): [value, neck, faces_z, faces_y, faces_x]})"""
    vol = np.asarray(vol)
    objects = cc.oracle_roots(vol, connectivity).reshape(-1).astype(np.int32).copy()
    flat_v = vol.reshape(-1)
    if values is None:
        values = [int(c) for c in np.unique(vol) if c != 0]
    report, contacts = {}, {}
    for value in values:
        components = len(set(objects[flat_v == value].tolist()))
        st = stages[value] if stages is not None else oracle_value(vol, value, connectivity)
        if st is None:
            report[value] = dict(components=components, separated=False)
            continue
        rep, merges = oracle_merge(st["rows"], st["peak_r"], depth)
        lowest = {}
        basin = st["basin"].tolist()
        for v in range(len(basin)):                                    # ascending: the first voxel of a set is its lowest
            if basin[v] >= 0:
                lowest.setdefault(rep[basin[v]], v)
        for v in range(len(basin)):
            if basin[v] >= 0:
                objects[v] = lowest[rep[basin[v]]]
        for (a, b), row in st["rows"].items():
            oa, ob = lowest[rep[a]], lowest[rep[b]]
            if oa != ob:
                c = contacts.setdefault((min(oa, ob), max(oa, ob)), [value, 0, 0, 0, 0])
                c[1] = max(c[1], row[0])
                for axis in range(3):
                    c[2 + axis] += row[1 + axis]
        report[value] = dict(components=components, separated=True, basins=len(st["peak_r"]), pair_rows=len(st["rows"]), merges=merges,
                             objects=len(set(lowest.values())))
    return objects, report, contacts


def rows_as_arrays(rows):
    """the dict of oracle_pairs sorted by key: (a, b, saddle, faces (rows, 3)) as int64"""
    keys = sorted(rows)
    table = np.array([[a, b] + rows[(a, b)] for a, b in keys], dtype=np.int64).reshape(-1, 6)
    return table[:, 0], table[:, 1], table[:, 2], table[:, 3:6]


# ---- the named scenes --------------------------------------------------------------------------------------------------------------
def _balls(shape, centres, radius, value=1):
    zi, yi, xi = np.indices(shape)
    vol = np.zeros(shape, dtype=np.uint8)
    for cz, cy, cx in centres:
        vol[(zi - cz) ** 2 + (yi - cy) ** 2 + (xi - cx) ** 2 <= radius * radius] = value
    return vol


def two_balls():
    """radius 8, centres 12 apart: two peaks and a neck"""
    return _balls((19, 19, 32), [(9, 9, 9), (9, 9, 21)], 8)


def three_balls():
    return _balls((13, 22, 24), [(6, 6, 6), (6, 6, 15), (6, 14, 11)], 5)


def cylinder():
    """an oblique cylinder of radius 4: a ridge whose sqrt(R) ripples, one object at any sensible depth"""
    shape = (14, 18, 40)
    zi, yi, xi = np.indices(shape).astype(np.float64)
    axis = np.array([0.2, 0.3, 1.0])
    axis /= np.linalg.norm(axis)
    rel = np.stack([zi - 7.0, yi - 9.0, xi - 20.0], axis=-1)
    along = rel @ axis
    d2 = (rel ** 2).sum(-1) - along ** 2
    return ((d2 <= 16.0) & (np.abs(along) <= 17.0)).astype(np.uint8)


def slab_z():
    """a solid slab whose mid-plane plateau (z = 4) crosses the 8 x 8 x 64 tile seams in y and x: long diagonal chains"""
    vol = np.zeros((9, 17, 130), dtype=np.uint8)
    vol[1:8, 1:16, 1:129] = 1
    return vol


def slab_y():
    """the same with the plateau across z and x seams"""
    vol = np.zeros((17, 9, 70), dtype=np.uint8)
    vol[1:16, 1:8, 1:69] = 1
    return vol


def rows_of(x):
    """blobs in rows that end before, on and after a 64-lane boundary"""
    return tc.blobs((5, 9, x), x)


def ties():
    """a box of even widths: every central voxel ties with its neighbours in R"""
    vol = np.zeros((6, 8, 12), dtype=np.uint8)
    vol[1:5, 1:7, 1:11] = 1
    return vol


def peak_on_face():
    """a ball cut by the face z = 0: outside the volume is not background, so the peak lies on the face"""
    return _balls((8, 15, 15), [(0, 7, 7)], 6)


def two_values():
    """values 1 and 2, each of them two touching balls, and the two values touch each other"""
    vol = _balls((13, 13, 40), [(6, 6, 6), (6, 6, 14)], 5, 1)
    other = _balls((13, 13, 40), [(6, 6, 24), (6, 6, 32)], 5, 2)
    vol[(other == 2) & (vol == 0)] = 2
    vol[6, 6, 19:21] = 2                                              # a bridge: the values touch
    return vol


SCENES = {
    "two_balls": two_balls, "three_balls": three_balls, "cylinder": cylinder, "slab_z": slab_z, "slab_y": slab_y,
    "rows_63": lambda: rows_of(63), "rows_64": lambda: rows_of(64), "rows_65": lambda: rows_of(65), "rows_130": lambda: rows_of(130),
    "plane": lambda: tc.blobs((1, 30, 34), 2), "line": tc.row, "ties": ties, "peak_on_face": peak_on_face, "two_values": two_values,
    "filled": tc.filled, "random": lambda: cc.random_labels((6, 7, 9), 3, 0.5, 4),
    "debris_rows": lambda: cc.random_labels((4, 6, 130), 2, 0.8, 5),     # more basins, and pairs of basins, per 64 voxels of a row than a wave groups by ballot
}
ABSENT = 9                                                             # a value no scene holds


def values_of(vol):
    return [int(c) for c in np.unique(vol) if c != 0]


@functools.lru_cache(maxsize=None)
def scene(name):
    vol = np.ascontiguousarray(SCENES[name]())
    vol.setflags(write=False)
    return vol


@functools.lru_cache(maxsize=None)
def stages_cached(name, value, connectivity):
    """oracle_value of a scene, computed once and left unchanged"""
    st = oracle_value(scene(name), value, connectivity)
    if st is not None:
        for key in ("r", "parent", "basin"):
            st[key].setflags(write=False)
    return st


def separate_cached(name, connectivity, depth, values=None):
    vol = scene(name)
    values = values_of(vol) if values is None else values
    return oracle_separate(vol, connectivity, depth, values, {value: stages_cached(name, value, connectivity) for value in values})


@functools.lru_cache(maxsize=None)
def vessels_expected():
    return json.loads(GOLDEN_VESSELS.read_text())


def record_vessels_fixture():
    """tests/golden/separation_vessels.json from the oracle alone: python tests/separation_cases.py"""
    vol = tc.vessels_crop()
    doc = {"crop": tc.CROP, "value": 255, "voxels": int((vol == 255).sum()), "connectivity": {}}
    for connectivity in cc.CONNECTIVITIES:
        st = oracle_value(vol, 255, connectivity)
        entry = {"basins": len(st["peak_r"]), "pair_rows": len(st["rows"]), "adjacent_pairs": st["count"], "objects": {}}
        for depth in DEPTHS:
            objects, report, contacts = oracle_separate(vol, connectivity, depth, [255], {255: st})
            roots, sizes = np.unique(objects[vol.reshape(-1) == 255], return_counts=True)
            entry["objects"][str(depth)] = {"count": report[255]["objects"], "merges": report[255]["merges"], "contacts": len(contacts),
                                            "roots": roots.tolist(), "voxels": sizes.tolist()}
        doc["connectivity"][str(connectivity)] = entry
    GOLDEN_VESSELS.write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    import sys
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    record_vessels_fixture()
