"""What the measurement tests share (tests/test_measurements_host.py, tests/test_hip_measurements.py): an oracle that uses neither
route of utilities/measurements.py - per component np.argwhere, plain int64 sums of the coordinates, and the exposed faces counted
on a volume padded with -1 by comparing every voxel with its two neighbours along an axis - a cross-check of that oracle with
scipy.ndimage where scipy imports, and the volumes the tests measure.  Roots come from components_cases.oracle_roots."""
import functools
import json

import numpy as np

import components_cases as cc

FIELDS = 20
GOLDEN_VESSELS = cc.GOLDEN / "measurements_vessels.json"


def exposed_faces(vol):
    """three uint8 arrays of vol.shape: per voxel the exposed faces across z, y, x (an axis of length 1 has none)"""
    vol = np.asarray(vol)
    padded = np.full(tuple(s + 2 for s in vol.shape), -1, dtype=np.int32)
    padded[1:-1, 1:-1, 1:-1] = vol
    centre = padded[1:-1, 1:-1, 1:-1]
    before = (padded[:-2, 1:-1, 1:-1], padded[1:-1, :-2, 1:-1], padded[1:-1, 1:-1, :-2])
    after = (padded[2:, 1:-1, 1:-1], padded[1:-1, 2:, 1:-1], padded[1:-1, 1:-1, 2:])
    return [((before[a] != centre).astype(np.uint8) + (after[a] != centre).astype(np.uint8)) if vol.shape[a] > 1 else np.zeros(vol.shape, np.uint8)
            for a in range(3)]


def oracle_rows(vol, comp, row_of_root, rows):
    """the (rows, 20) int64 table vs_component_moments writes for the row assignment `row_of_root` (one int per voxel index, -1 = not
    measured), component by component; a row nothing maps to holds 0 voxels and the empty box"""
    vol, comp = np.asarray(vol), np.asarray(comp)
    row_of_root = np.asarray(row_of_root).reshape(-1)
    table = np.zeros((rows, FIELDS), dtype=np.int64)
    table[:, 10], table[:, 12], table[:, 14] = vol.shape
    table[:, 11] = table[:, 13] = table[:, 15] = -1
    faces = exposed_faces(vol)
    for root in np.unique(comp).tolist():
        row = int(row_of_root[root])
        if row < 0:
            continue
        at = np.argwhere(comp == root).astype(np.int64)
        z, y, x = at[:, 0], at[:, 1], at[:, 2]
        inside = comp == root
        touches = any(vol.shape[a] > 1 and ((at[:, a] == 0) | (at[:, a] == vol.shape[a] - 1)).any() for a in range(3))
        table[row] = [len(at), z.sum(), y.sum(), x.sum(), (z * z).sum(), (y * y).sum(), (x * x).sum(), (z * y).sum(), (z * x).sum(), (y * x).sum(),
                      z.min(), z.max(), y.min(), y.max(), x.min(), x.max(),
                      int(faces[0][inside].sum(dtype=np.int64)), int(faces[1][inside].sum(dtype=np.int64)), int(faces[2][inside].sum(dtype=np.int64)),
                      int(touches)]
    return table


def oracle_selection(vol, comp, min_voxels=1, background=0, include_background=False):
    """(roots of the measured components by value then root, their values, row_of_root, not-listed objects and voxels per value)"""
    flat_v, flat_c = np.asarray(vol).reshape(-1), np.asarray(comp).reshape(-1)
    listed, objects, voxels = [], np.zeros(256, np.int64), np.zeros(256, np.int64)
    for root, count in zip(*np.unique(flat_c, return_counts=True)):
        value = int(flat_v[root])
        if count < min_voxels or (value == background and not include_background):
            objects[value] += 1
            voxels[value] += count
        else:
            listed.append((value, int(root)))
    listed.sort()
    row_of_root = np.full(flat_c.size, -1, dtype=np.int32)
    for row, (_, root) in enumerate(listed):
        row_of_root[root] = row
    return (np.array([r for _, r in listed], dtype=np.int64), np.array([v for v, _ in listed], dtype=np.int64), row_of_root, objects, voxels)


def oracle_measure(vol, connectivity, min_voxels=1, background=0, include_background=False, roots=None):
    """what measure_components returns, from the oracles"""
    vol = np.asarray(vol)
    comp = cc.oracle_roots(vol, connectivity) if roots is None else np.asarray(roots)
    listed, values, row_of_root, objects, voxels = oracle_selection(vol, comp, min_voxels, background, include_background)
    return dict(table=oracle_rows(vol, comp, row_of_root, len(listed)), roots=listed, values=values, not_listed_objects=objects,
                not_listed_voxels=voxels, shape=np.array(vol.shape, dtype=np.int64))


def assert_raw_equal(got, want, what=""):
    for name in ("roots", "values", "table", "not_listed_objects", "not_listed_voxels", "shape"):
        a, b = np.asarray(got[name]), np.asarray(want[name])
        assert a.dtype == np.int64 and a.shape == b.shape and np.array_equal(a, b), (what, name, a, b)


def scipy_cross_check(vol, comp, raw):
    """voxels, coordinate sums and bounding boxes of `raw` from scipy.ndimage.sum_labels / find_objects; False where scipy does not import"""
    try:
        from scipy import ndimage
    except ImportError:
        return False
    vol, comp = np.asarray(vol), np.asarray(comp)
    labelled = np.zeros(vol.shape, dtype=np.int32)
    for row, root in enumerate(raw["roots"].tolist()):
        labelled[comp == root] = row + 1
    index = np.arange(1, len(raw["roots"]) + 1)
    if len(index) == 0:
        return True
    grid = np.indices(vol.shape)
    assert np.array_equal(ndimage.sum_labels(np.ones(vol.shape), labelled, index).astype(np.int64), raw["table"][:, 0])
    for a in range(3):
        assert np.array_equal(np.rint(ndimage.sum_labels(grid[a].astype(np.float64), labelled, index)).astype(np.int64), raw["table"][:, 1 + a])
    for row, box in enumerate(ndimage.find_objects(labelled)):
        assert [b for s in box for b in (s.start, s.stop - 1)] == raw["table"][row, 10:16].tolist()
    return True


# ---- volumes ---------------------------------------------------------------------------------------------------------------------
DEGENERATE_SHAPES = [(1, 1, 1), (7, 1, 5), (3, 4, 1), (1, 1, 37)]


def box_in_volume(shape=(12, 14, 20), at=(3, 4, 5), box=(2, 3, 4), value=1):
    vol = np.zeros(shape, dtype=np.uint8)
    vol[at[0]:at[0] + box[0], at[1]:at[1] + box[1], at[2]:at[2] + box[2]] = value
    return vol


def alternating_x(shape=(4, 8, 130)):
    """values 1 and 2 voxel by voxel along x, every row alike but the first of a plane (all 1) and the last (all 2), which join the columns
    of their value: two components, runs of length 1 nearly everywhere"""
    vol = np.zeros(shape, dtype=np.uint8)
    vol[:] = 1 + np.arange(shape[2]) % 2
    vol[:, 0, :], vol[:, -1, :] = 1, 2
    return vol


def stripes_y(shape=(2, 80, 70), count=40):
    """`count` stripes of two rows each along y with distinct values 1 .. count: more components in a wave's span than its cache holds"""
    vol = np.zeros(shape, dtype=np.uint8)
    vol[:] = (1 + np.arange(shape[1]) // (shape[1] // count))[None, :, None]
    return vol


def three_runs(shape=(1, 2, 70000)):
    """two rows of 70000 voxels cut into three runs each at x = 20000 and x = 65536: sums of x^2 beyond 2^32 and closed forms at large x"""
    vol = np.ones(shape, dtype=np.uint8)
    vol[:, :, 20000:65536] = 2
    vol[:, :, 65536:] = 3
    return vol


@functools.lru_cache(maxsize=None)
def vessels_expected():
    return json.loads(GOLDEN_VESSELS.read_text())


def write_vessels_golden():
    """tests/golden/measurements_vessels.json from the oracle alone: the raw integers of the vessels fixture, background
    included, under connectivity 6 and 26"""
    doc = {}
    for connectivity in (6, 26):
        raw = oracle_measure(cc.vessels(), connectivity, include_background=True)
        doc[str(connectivity)] = {"roots": raw["roots"].tolist(), "values": raw["values"].tolist(), "table": raw["table"].tolist(),
                                  "not_listed": {str(v): [int(raw["not_listed_objects"][v]), int(raw["not_listed_voxels"][v])]
                                                 for v in np.flatnonzero(raw["not_listed_objects"])}}
    GOLDEN_VESSELS.write_text(json.dumps(doc, separators=(",", ":")) + "\n")


if __name__ == "__main__":              # python tests/measurement_cases.py (from the repository root) writes the golden file again
    write_vessels_golden()
