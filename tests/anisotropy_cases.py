"""What the anisotropic-voxel tests share (tests/test_anisotropy_host.py, tests/test_hip_anisotropy.py), NumPy only and neither
route of the code under test: the brute-force oracle on a grid whose steps along z, y, x are the integer weights w.

R: three weighted int64 min-plus passes, out(p) = min over p' of f(p') + q (p - p')^2 with q = w^2, the squares from index
differences.  T2: EVERY voxel of the value is a centre and every voxel u with D(u - v) < R(v), D = qz dz^2 + qy dy^2 + qx dx^2, is
painted with the maximum, voxel by voxel - nothing is pruned, nothing is a span.  Surface scores: float64 straight from the
coordinates times the FLOAT spacing, sqrt((sz dz)^2 + (sy dy)^2 + (sx dx)^2) between every pair of surface voxels - never through
the weights or a histogram."""
import functools

import numpy as np

import surface_cases as sc
import thickness_cases as tc

INF = 0xFFFFFFFF
WEIGHTS = ((3, 1, 1), (5, 2, 2), (1, 2, 3), (2, 1, 4))           # coarse z; a unit below 1; every axis different; coarse x


# ---- integers ----------------------------------------------------------------------------------------------------------------------
def weighted_d2(seeds, weights):
    """uint32 (Z, Y, X): the least qz dz^2 + qy dy^2 + qx dx^2 to a non-zero voxel of `seeds`, 0xFFFFFFFF when there is none"""
    seeds = np.asarray(seeds) != 0
    assert seeds.ndim == 3
    big = np.int64(1) << 50
    d = np.where(seeds, np.int64(0), big)
    for axis in range(3):
        q = np.int64(int(weights[axis]) ** 2)
        length = d.shape[axis]
        pos = np.arange(length, dtype=np.int64)
        f = np.moveaxis(d, axis, 0)
        out = np.empty_like(f)
        for p in range(length):
            out[p] = (f + (q * (pos - p) ** 2).reshape(-1, 1, 1)).min(axis=0)
        d = np.moveaxis(out, 0, axis)
    return np.where(d >= big, INF, d).astype(np.uint32)


def exact_r(vol, value, weights):
    """int64 (Z, Y, X): R of the voxels of `value` on the weighted grid, 0 off the value; None when there is no other value"""
    member = np.asarray(vol) == value
    if member.all():
        return None
    return np.where(member, weighted_d2(~member, weights).astype(np.int64), 0)


def oracle_t2(vol, value, weights):
    """uint32 (Z, Y, X): T2 of `value` by painting the ball of every voxel of the value, voxel by voxel"""
    vol = np.asarray(vol)
    r = exact_r(vol, value, weights)
    t2 = np.zeros(vol.shape, dtype=np.int64)
    if r is None:
        return t2.astype(np.uint32)
    qz, qy, qx = (int(w) ** 2 for w in weights)
    big_z, big_y, big_x = vol.shape
    for z, y, x in zip(*np.nonzero(r)):
        rv = int(r[z, y, x])
        hz, hy, hx = (int(np.sqrt(rv / q)) + 1 for q in (qz, qy, qx))   # generous: q (h + 1)^2 > R, and the comparison below decides
        z0, z1, y0, y1, x0, x1 = max(z - hz, 0), min(z + hz, big_z - 1), max(y - hy, 0), min(y + hy, big_y - 1), max(x - hx, 0), min(x + hx, big_x - 1)
        d = (qz * (np.arange(z0, z1 + 1) - z) ** 2)[:, None, None] + (qy * (np.arange(y0, y1 + 1) - y) ** 2)[None, :, None] \
            + (qx * (np.arange(x0, x1 + 1) - x) ** 2)[None, None, :]
        box = t2[z0:z1 + 1, y0:y1 + 1, x0:x1 + 1]
        np.maximum(box, np.where(d < rv, rv, 0), out=box)
    return t2.astype(np.uint32)


@functools.lru_cache(maxsize=None)
def t2_cached(name, value, weights):
    t2 = oracle_t2(tc.VOLUMES[name](), value, weights)
    t2.setflags(write=False)
    return t2


def histograms_np(pred, truth_classes, classes, weights, ignored=None):
    """what surface_distance_histograms returns under a spacing: indexed by the weighted integers"""
    return sc.histograms_np(pred, truth_classes, classes, ignored, d2=lambda seeds: weighted_d2(seeds, weights))


# ---- floats from coordinates -------------------------------------------------------------------------------------------------------
def _nearest(points, others, spacing):
    """float64: for every row of `points` the distance to the nearest row of `others`, coordinates times the spacing"""
    a = points.astype(np.float64) * np.asarray(spacing, dtype=np.float64)
    b = others.astype(np.float64) * np.asarray(spacing, dtype=np.float64)
    out = np.empty(len(a))
    chunk = max(1, (1 << 22) // max(len(b), 1))
    for i in range(0, len(a), chunk):
        out[i:i + chunk] = np.sqrt(((a[i:i + chunk, None, :] - b[None, :, :]) ** 2).sum(2)).min(1)
    return out


def coordinate_scores(pred, truth_classes, classes, spacing, tolerance, ignored=None):
    """the figures of `surface_cases.brute_surface_scores`, with every distance from coordinates times the float spacing"""
    names = ("hausdorff", "hausdorff_95", "assd", "mean_distance_truth_to_pred", "mean_distance_pred_to_truth", "surface_dice")
    out = {n: [] for n in names + sc.INTEGER_FIGURES}
    for c in range(classes):
        a, b = sc.class_masks(pred, truth_classes, c, ignored)
        sa, sb = np.argwhere(sc.surface_np(a)), np.argwhere(sc.surface_np(b))
        out["truth_surface_voxels"].append(len(sa))
        out["predicted_surface_voxels"].append(len(sb))
        if len(sa) + len(sb) == 0:
            figures, within = [float("nan")] * 6, (0, 0)
        elif len(sa) == 0 or len(sb) == 0:
            figures, within = [float("inf")] * 5 + [0.0], (0, 0)
        else:
            dtp, dpt = _nearest(sa, sb, spacing), _nearest(sb, sa, spacing)
            pooled = np.concatenate([dtp, dpt])
            within = (int((dtp <= tolerance).sum()), int((dpt <= tolerance).sum()))
            figures = [float(pooled.max()), float(np.percentile(pooled, 95)), float(np.mean(pooled)), float(np.mean(dtp)), float(np.mean(dpt)),
                       (within[0] + within[1]) / pooled.size]
        for n, v in zip(names, figures):
            out[n].append(v)
        out["truth_within_tolerance"].append(within[0])
        out["predicted_within_tolerance"].append(within[1])
    present = [c for c in range(classes) if out["truth_surface_voxels"][c] + out["predicted_surface_voxels"][c]]
    for n, m in (("hausdorff", "mean_hausdorff"), ("hausdorff_95", "mean_hausdorff_95"), ("assd", "mean_assd"), ("surface_dice", "mean_surface_dice")):
        out[m] = float(np.mean([out[n][c] for c in present])) if present else float("nan")
    return out


def assert_scores_equal(s, b):
    """integers exactly; float figures within 1e-12 relative of the coordinate oracle"""
    for name in sc.INTEGER_FIGURES:
        assert np.asarray(getattr(s, name)).tolist() == b[name], name
    for name in sc.FLOAT_FIGURES + ("surface_dice",):
        np.testing.assert_allclose(getattr(s, name), np.array(b[name]), rtol=1e-12, atol=0, equal_nan=True, err_msg=name)
    for name in ("mean_hausdorff", "mean_hausdorff_95", "mean_assd", "mean_surface_dice"):
        np.testing.assert_allclose(getattr(s, name), b[name], rtol=1e-12, atol=0, equal_nan=True, err_msg=name)


# ---- volumes ---------------------------------------------------------------------------------------------------------------------
SPACINGS = {"z_coarse": ([2.5, 1.0, 1.0], 1.3), "all_differ": ([1.0, 2.0, 3.0], 2.5)}      # spacing, a tolerance no distance of the grid equals


@functools.lru_cache(maxsize=None)
def scored_pair():
    """(pred, truth classes, raw truth with an ignored band, its ignored mask) on a small coherent pair: class 3 is in the truth
    only (every distance figure inf), class 4 in neither (NaN)"""
    pred, truth = (a.copy() for a in sc.coherent_pair((8, 14, 20), 3, 12))
    pred[pred == 3] = 2
    raw = np.array([0, 7, 100, 200, 201], dtype=np.uint8)[truth]
    raw[:, 6:8, :] = 255
    for a in (pred, truth, raw):
        a.setflags(write=False)
    return pred, truth, raw, raw == 255


LABEL_VALUES = [0, 7, 100, 200, 201]


def physical_ball():
    """a physical ball of radius 12 sampled at spacing (3, 1, 1): 13 x 31 x 31, centre (6, 15, 15), 2353 voxels"""
    z, y, x = np.indices((13, 31, 31))
    return (((3 * (z - 6)) ** 2 + (y - 15) ** 2 + (x - 15) ** 2) <= 144).astype(np.uint8)


def corner_seed(shape):
    seeds = np.zeros(shape, dtype=np.uint8)
    seeds[0, 0, 0] = 1
    return seeds


def axis_one_volume(shape):
    """the volumes of the axis-of-1 thickness tests of tests/test_hip_thickness.py"""
    vol = (tc._smooth_field(shape, 7) > 0.45).astype(np.uint8)
    vol[..., -1] = 1
    vol[..., 5] = 0
    return vol


# ---- separation ------------------------------------------------------------------------------------------------------------------
PACKINGS = ("two_balls", "three_balls", "two_values", "rows_65")        # small scenes of tests/separation_cases.py


@functools.lru_cache(maxsize=None)
def separation_stages(name, value, weights, connectivity=6):
    """the depth-independent stages of `separation_cases.oracle_value` on the weighted distance map"""
    import separation_cases as spc
    vol = spc.scene(name)
    r = exact_r(vol, value, weights)
    if r is None or not (np.asarray(vol) == value).any():
        return None
    parent = spc.oracle_parents(r, connectivity)
    basin = spc.oracle_basins(parent)
    rows, count = spc.oracle_pairs(r, basin, connectivity)
    peaks = np.flatnonzero(basin == np.arange(basin.size))
    return dict(r=r, parent=parent, basin=basin, rows=rows, count=count, peak_r={int(p): int(r.reshape(-1)[p]) for p in peaks})


def oracle_separate(name, weights, depth, connectivity=6):
    """`separation_cases.oracle_separate` on the weighted grid.  The depth is in voxels of the finest axis: (sqrt(H) - sqrt(S)) / w_min <
    depth, which for the weights used here (w_min 1 or 2: an exact division) is the oracle's sqrt(H) - sqrt(S) < depth * w_min."""
    import separation_cases as spc
    assert min(weights) in (1, 2, 4)
    vol = spc.scene(name)
    stages = {value: separation_stages(name, value, weights, connectivity) for value in spc.values_of(vol)}
    return spc.oracle_separate(vol, connectivity, depth * min(weights), None, stages)


def assert_separation_equals_oracle(got, name, weights, depth, connectivity=6):
    """objects, report and contacts of `separate_objects` against the oracle"""
    objects, report, contacts = oracle_separate(name, weights, depth, connectivity)
    assert np.array_equal(got["objects"].reshape(-1), objects)
    for value, want in report.items():
        have = got["report"][str(value)]
        assert {k: have[k] for k in want} == want, value
    keys = sorted(contacts, key=lambda k: (contacts[k][0], k))
    c = got["contacts"]
    assert list(zip(c["root_a"].tolist(), c["root_b"].tolist())) == keys
    assert c["value"].tolist() == [contacts[k][0] for k in keys] and c["neck_squared"].tolist() == [contacts[k][1] for k in keys]
    assert c["faces"].tolist() == [contacts[k][2:5] for k in keys]
