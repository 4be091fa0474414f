"""What the local-thickness tests share, and neither route of utilities/thickness.py: the brute-force oracle, a second formulation
through scipy's distance transform, the named volumes and the committed figures of a crop of the vessels fixture.

Oracle: R by three exact min-plus passes over integer index differences; then EVERY voxel of the value is a centre and every voxel
within |u - v|^2 < R(v), with the squares taken from index differences, is painted with the maximum.  Nothing is pruned and nothing
is a span."""
import functools
import json
from pathlib import Path

import numpy as np

import components_cases as cc

GOLDEN = Path(__file__).resolve().parent / "golden"
INF_R = 0xFFFFFFFF
CROP = {"offset": [176, 160, 16], "shape": [48, 64, 64]}     # of the vessels fixture; tests/golden/thickness_vessels.json records it too


# ---- the oracle --------------------------------------------------------------------------------------------------------------------
def exact_r(vol, value):
    """int64 (Z, Y, X): the squared distance of every voxel of `value` to the nearest in-volume voxel of another value, 0 off the value;
    None when there is no other value"""
    member = np.asarray(vol) == value
    if member.all():
        return None
    big = np.int64(1) << 40
    d = np.where(member, big, np.int64(0))
    for axis in range(3):
        length = d.shape[axis]
        pos = np.arange(length, dtype=np.int64)
        f = np.moveaxis(d, axis, 0)
        out = np.empty_like(f)
        for p in range(length):
            out[p] = (f + ((pos - p) ** 2).reshape(-1, 1, 1)).min(axis=0)
        d = np.moveaxis(out, 0, axis)
    return np.ascontiguousarray(d)


def oracle_t2(vol, value):
    """uint32 (Z, Y, X): T2 of `value` by painting the ball of every voxel of the value, voxel by voxel"""
    vol = np.asarray(vol)
    r = exact_r(vol, value)
    t2 = np.zeros(vol.shape, dtype=np.int64)
    if r is None:
        return t2.astype(np.uint32)
    big_z, big_y, big_x = vol.shape
    for z, y, x in zip(*np.nonzero(r)):
        rv = int(r[z, y, x])
        h = int(np.sqrt(rv)) + 1                                       # generous: the comparison below decides
        z0, z1, y0, y1, x0, x1 = max(z - h, 0), min(z + h, big_z - 1), max(y - h, 0), min(y + h, big_y - 1), max(x - h, 0), min(x + h, big_x - 1)
        d2 = ((np.arange(z0, z1 + 1) - z) ** 2)[:, None, None] + ((np.arange(y0, y1 + 1) - y) ** 2)[None, :, None] \
            + ((np.arange(x0, x1 + 1) - x) ** 2)[None, None, :]
        box = t2[z0:z1 + 1, y0:y1 + 1, x0:x1 + 1]
        np.maximum(box, np.where(d2 < rv, rv, 0), out=box)
    return t2.astype(np.uint32)


def scipy_t2(vol, value):
    """the second formulation: T2(u) = the largest rho such that the squared distance from u to {v : R(v) = rho} is below rho, one scipy
    transform per distinct rho; None where scipy does not import"""
    try:
        from scipy import ndimage
    except ImportError:
        return None
    vol = np.asarray(vol)
    r = exact_r(vol, value)
    t2 = np.zeros(vol.shape, dtype=np.int64)
    if r is None:
        return t2.astype(np.uint32)
    for rho in np.unique(r[r > 0]).tolist():
        d2 = np.rint(ndimage.distance_transform_edt(r != rho) ** 2).astype(np.int64)
        t2[d2 < rho] = rho                                             # ascending rho: the largest stays
    return t2.astype(np.uint32)


def oracle_centres_all(vol, value):
    """every voxel of the value, as sorted linear indices: the list a route that drops nothing would paint"""
    return np.flatnonzero(np.asarray(vol).reshape(-1) == value)


# ---- the named volumes -------------------------------------------------------------------------------------------------------------
def _smooth_field(shape, seed):
    rng = np.random.default_rng(seed)
    f = rng.random(shape)
    for axis, extent in enumerate(shape):
        if extent > 1:
            for _ in range(3):
                f = (np.roll(f, 1, axis) + f + np.roll(f, -1, axis)) / 3.0
    return f


def blobs(shape=(12, 14, 16), seed=1):
    f = _smooth_field(shape, seed)
    return (f > np.median(f)).astype(np.uint8)


def row():
    v = np.zeros((1, 1, 40), np.uint8)
    v[0, 0, 3:12] = 1
    v[0, 0, 25:] = 1                 # reaches the end of the row
    return v


def disc_prism(shape=(4, 80, 80), radius=36):
    _, yi, xi = np.indices(shape)
    return (((yi - 40) ** 2 + (xi - 40) ** 2) <= radius * radius).astype(np.uint8)


def long_box():
    v = np.zeros((5, 9, 80), np.uint8)
    v[1:4, 2:7, 5:75] = 1            # 3 x 5 x 70
    return v


def debris():
    return cc.random_labels((10, 12, 13), 2, 0.7, 5)


def touching():
    v = np.zeros((9, 12, 20), np.uint8)
    v[2:7, 2:10, 2:10] = 1
    v[2:7, 3:9, 10:18] = 2           # touches value 1 along x = 9 | 10
    return v


def single_voxel():
    v = np.zeros((5, 5, 5), np.uint8)
    v[2, 2, 2] = 1
    return v


def filled():
    return np.full((4, 5, 6), 3, np.uint8)


def vessels_crop():
    (z, y, x), (dz, dy, dx) = CROP["offset"], CROP["shape"]
    return np.ascontiguousarray(cc.vessels()[z:z + dz, y:y + dy, x:x + dx])


def slab(x):
    """a thick slab over whole rows of length x and a thinner bar that stops 3 voxels short of the row's end: spans end before, on and
    after a 64-lane boundary and are clipped at both ends of the row"""
    v = np.zeros((9, 11, x), np.uint8)
    v[1:8, 1:10, :] = 1
    v[8, 4:7, 2:x - 3] = 1
    return v


VOLUMES = {"blobs": blobs, "blobs_2d": lambda: blobs((1, 30, 34), 2), "row": row, "disc_prism": disc_prism, "long_box": long_box, "debris": debris,
           "touching": touching, "single_voxel": single_voxel, "filled": filled, "vessels_crop": vessels_crop}


def values_of(vol):
    return [int(c) for c in np.unique(vol).tolist() if c != 0]


@functools.lru_cache(maxsize=None)
def oracle_cached(name, value):
    t2 = oracle_t2(VOLUMES[name](), value)
    t2.setflags(write=False)
    return t2


@functools.lru_cache(maxsize=None)
def vessels_expected():
    return json.loads((GOLDEN / "thickness_vessels.json").read_text())


def numpy_figures(t2, member, voxel_size):
    """the figures from the expanded thicknesses, by NumPy"""
    d = 2.0 * voxel_size * np.sqrt(t2[member].astype(np.float64))
    return {"voxels": int(member.sum()), "mean": float(d.mean()), "std": float(d.std()), "min": float(d.min()), "max": float(d.max()),
            "median": float(np.median(d)), "p5": float(np.percentile(d, 5)), "p95": float(np.percentile(d, 95))}


def record_vessels_fixture():
    """tests/golden/thickness_vessels.json from the oracle alone: python tests/thickness_cases.py"""
    vol = vessels_crop()
    t2, r = oracle_t2(vol, 255), exact_r(vol, 255)
    used, counts = np.unique(t2[vol == 255], return_counts=True)
    doc = {"crop": CROP, "value": 255, "voxel_size": 1.0, "max_squared_radius": int(r.max()),
           "histogram": {"squared_thickness": used.tolist(), "count": counts.tolist()},
           "figures": dict(numpy_figures(t2, vol == 255, 1.0), largest_inscribed_diameter=2.0 * float(np.sqrt(float(r.max()))))}
    (GOLDEN / "thickness_vessels.json").write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    import sys
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    record_vessels_fixture()
