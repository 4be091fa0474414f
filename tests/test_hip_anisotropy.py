"""-m gpu: the kernels behind voxel_spacing - vs_edt_squared_scaled (csrc/surface.hip) and vs_thickness_centres_scaled / _paint_scaled /
_resolve_scaled (csrc/thickness.hip) through the C ABI, integer for integer against the brute-force oracle of
tests/anisotropy_cases.py, at every size where the kernels take another path; then the Python routes on the device against the host
routes and the oracles (surface distances, thickness, separation), and the manager with the key.  Buffers start out full of
garbage; nothing here has a tolerance except float figures against distances computed from coordinates (1e-12 relative)."""
import json
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import anisotropy_cases as ac
import separation_cases as spc
import thickness_cases as tc
from hip_helpers import DEV, lib
from volume_segmantics_amd.utilities import label_volume as lv
from volume_segmantics_amd.utilities import separation as sp
from volume_segmantics_amd.utilities import surface_distance as sd
from volume_segmantics_amd.utilities import thickness as th

pytestmark = pytest.mark.gpu

GARBAGE32 = -0x01234567
GARBAGE64 = -0x0123456789ABCDEF
EDT_WEIGHTS = ac.WEIGHTS + ((64, 1, 1),)


# ---- the transform through the C ABI -------------------------------------------------------------------------------------------------
def run_edt(seeds, weights=None):
    """vs_edt_squared_scaled (vs_edt_squared for weights None) into garbage: uint32 (Z, Y, X) on the host"""
    L = lib()
    seeds = np.asarray(seeds)
    shape = tuple(seeds.shape)
    s = torch.from_numpy((seeds != 0).astype(np.uint8).reshape(-1)).to(DEV)
    d2 = torch.full((s.numel() + 4,), GARBAGE32, dtype=torch.int32, device=DEV)
    need = L.lib.vs_edt_workspace_bytes(*shape)
    work = torch.full((need,), 0xA5, dtype=torch.uint8, device=DEV)
    if weights is None:
        L.check(L.lib.vs_edt_squared(L.ptr(s), *shape, L.ptr(d2), L.ptr(work) if need else None, need, L.stream_ptr()))
    else:
        L.check(L.lib.vs_edt_squared_scaled(L.ptr(s), *shape, *weights, L.ptr(d2), L.ptr(work) if need else None, need, L.stream_ptr()))
    torch.cuda.synchronize()
    assert (d2[-4:] == GARBAGE32).all()                                # nothing behind the volume is touched
    return d2[:-4].cpu().numpy().view(np.uint32).reshape(shape)


EDT_VOLUMES = {"blobs": lambda: tc.blobs() == 0, "debris": lambda: tc.debris() == 0, "touching": lambda: tc.touching() == 1,
               "seedless": lambda: np.zeros((5, 6, 70), bool), "corner": lambda: ac.corner_seed((6, 9, 11)),
               "x63": lambda: tc.blobs((5, 6, 63), 3) == 0, "x64": lambda: tc.blobs((5, 6, 64), 4) == 0, "x65": lambda: tc.blobs((5, 6, 65), 5) == 0,
               "x130": lambda: tc.blobs((4, 5, 130), 6) == 0, "1x1x130": lambda: tc.blobs((1, 1, 130), 7) == 0,
               "7x1x70": lambda: tc.blobs((7, 1, 70), 8) == 0, "1x9x66": lambda: tc.blobs((1, 9, 66), 9) == 0}


@pytest.mark.parametrize("name", sorted(EDT_VOLUMES))
def test_transform_against_the_oracle(name):
    seeds = EDT_VOLUMES[name]()
    if name == "seedless":
        assert (run_edt(seeds, (3, 1, 1)) == ac.INF).all()
    for weights in EDT_WEIGHTS:
        assert np.array_equal(run_edt(seeds, weights), ac.weighted_d2(seeds, weights)), weights


@pytest.mark.parametrize("shape", [(520, 3, 66), (3, 520, 66)])
def test_global_memory_passes(shape):
    """an axis longer than the LDS tile: one corner seed, so the answer is the weighted squared coordinates"""
    z, y, x = np.indices(shape).astype(np.int64)
    for weights in ((3, 1, 1), (1, 2, 3), (2, 5, 1)):
        want = weights[0] ** 2 * z * z + weights[1] ** 2 * y * y + weights[2] ** 2 * x * x
        assert np.array_equal(run_edt(ac.corner_seed(shape), weights), want.astype(np.uint32)), weights
    far = np.zeros(shape, np.uint8)
    far[-1, -1, -1] = far[shape[0] // 2, shape[1] // 2, 7] = 1           # searches that run the other way and meet in the middle
    assert np.array_equal(run_edt(far, (2, 1, 4)), ac.weighted_d2(far, (2, 1, 4)))


def test_unit_and_common_weights_and_transposition():
    seeds = tc.blobs((9, 12, 70), 11) == 0
    plain = run_edt(seeds)
    assert np.array_equal(run_edt(seeds, (1, 1, 1)), plain)
    for k in (2, 7, 64):                                                # the C entry takes a common factor: k^2 times the plain transform
        assert np.array_equal(run_edt(seeds, (k, k, k)), (k * k) * plain)
    for axes, weights in (((2, 0, 1), (3, 1, 2)), ((1, 0, 2), (2, 1, 3)), ((2, 1, 0), (3, 2, 1))):
        moved = run_edt(np.ascontiguousarray(seeds.transpose(axes)), weights)
        back = np.argsort(axes)
        assert np.array_equal(moved.transpose(back), run_edt(seeds, (1, 2, 3))), axes


def test_transform_refusals_come_before_any_launch():
    L = lib()
    P, S = L.ptr, L.stream_ptr()
    a = torch.zeros(64, dtype=torch.int32, device=DEV)
    assert L.lib.vs_edt_squared_scaled(P(a), 1025, 1, 1, 64, 1, 1, P(a), None, 0, S) == -1 and "2^32 - 1" in L.last_error()
    assert L.lib.vs_edt_squared_scaled(P(a), 1, 1, 1025, 1, 1, 64, P(a), None, 0, S) == -1 and "2^32 - 1" in L.last_error()
    for weights in ((0, 1, 1), (1, 65, 1), (1, 1, -3)):
        assert L.lib.vs_edt_squared_scaled(P(a), 2, 2, 2, *weights, P(a), None, 0, S) == -1 and "1..64" in L.last_error(), weights
        assert L.lib.vs_thickness_workspace_bytes_scaled(2, 2, 2, *weights, 5) == 0
        assert L.lib.vs_thickness_centres_scaled(P(a), 2, 2, 2, *weights, None, 0, P(a), 4, P(a), S) == -1 and "1..64" in L.last_error()
        assert L.lib.vs_thickness_paint_scaled(P(a), 2, 2, 2, *weights, P(a), 1, 5, 5, P(a), 64, 1, S) == -1 and "1..64" in L.last_error()
        assert L.lib.vs_thickness_resolve_scaled(P(a), 2, 2, 2, *weights, 1, 5, P(a), 64, P(a), S) == -1 and "1..64" in L.last_error()
    assert L.lib.vs_thickness_workspace_bytes_scaled(1025, 1, 1, 64, 1, 1, 5) == 0
    assert L.lib.vs_edt_squared_scaled(None, 2, 2, 2, 1, 2, 3, P(a), None, 0, S) == -1 and "null" in L.last_error()
    torch.cuda.synchronize()
    assert not a.any()                                                  # nothing ran
    with pytest.raises(ValueError, match="2\\^32 - 1"):
        sd.squared_distance_transform(torch.zeros((1025, 1, 1), dtype=torch.uint8, device=DEV), spacing=[64, 1, 1])


# ---- thickness through the C ABI -----------------------------------------------------------------------------------------------------
def run_r(vol, value, weights):
    L = lib()
    shape = tuple(vol.shape)
    seeds = torch.from_numpy((np.asarray(vol) != value).astype(np.uint8).reshape(-1)).to(DEV)
    r = torch.full((seeds.numel(),), GARBAGE32, dtype=torch.int32, device=DEV)
    need = L.lib.vs_edt_workspace_bytes(*shape)
    work = torch.empty(need, dtype=torch.uint8, device=DEV)
    L.check(L.lib.vs_edt_squared_scaled(L.ptr(seeds), *shape, *weights, L.ptr(r), L.ptr(work) if need else None, need, L.stream_ptr()))
    return r


def run_centres(r, shape, weights, need):
    """(the centre list as it came, [centres, row spans]); one slot of garbage behind the list must stay"""
    L = lib()
    capacity = int((r != 0).sum())
    centres = torch.full((capacity + 1,), GARBAGE32, dtype=torch.int32, device=DEV)
    totals = torch.full((2,), GARBAGE64, dtype=torch.int64, device=DEV)
    table = None if need is None else torch.from_numpy(np.ascontiguousarray(need).view(np.int32)).to(DEV)
    L.check(L.lib.vs_thickness_centres_scaled(L.ptr(r), *shape, *weights, L.ptr(table), 0 if need is None else need.shape[1], L.ptr(centres), capacity,
                                              L.ptr(totals), L.stream_ptr()))
    torch.cuda.synchronize()
    count, rows = totals.cpu().tolist()
    assert 0 <= count <= capacity and int(centres[-1]) == GARBAGE32
    return centres[:count].clone(), [count, rows]


def run_paint_resolve(labels, r, shape, weights, value, centres, max_r, pieces=1):
    """(the K levels after the resolve, T2); the centre list goes in `pieces` calls"""
    L = lib()
    n = r.numel()
    need = L.lib.vs_thickness_workspace_bytes_scaled(*shape, *weights, max_r)
    levels = th.table_levels(shape[2], max_r, weights[2] ** 2)
    assert need == 4 * levels * n
    work = torch.full((need + 16,), 0xA5, dtype=torch.uint8, device=DEV)
    count = centres.numel()
    cuts = [count * i // pieces for i in range(pieces + 1)]
    for i in range(pieces):
        L.check(L.lib.vs_thickness_paint_scaled(L.ptr(r), *shape, *weights, centres.data_ptr() + 4 * cuts[i], cuts[i + 1] - cuts[i], max_r, max_r,
                                                L.ptr(work), need, int(i == 0), L.stream_ptr()))
    t2 = torch.full((n,), GARBAGE32, dtype=torch.int32, device=DEV)
    L.check(L.lib.vs_thickness_resolve_scaled(L.ptr(labels), *shape, *weights, value, max_r, L.ptr(work), need, L.ptr(t2), L.stream_ptr()))
    torch.cuda.synchronize()
    assert (work[need:] == 0xA5).all()                                   # nothing behind the table is touched
    return work[:need].view(torch.int32).reshape(levels, n).cpu().numpy().view(np.uint32), t2


def assert_thickness(vol, value, weights, want=None, pieces=1):
    """the three scaled kernels against the oracle (and, level for level, against the host's table of the same centres)"""
    vol = np.asarray(vol)
    shape = tuple(vol.shape)
    r_want = ac.exact_r(vol, value, weights).astype(np.uint32)
    want = ac.oracle_t2(vol, value, weights) if want is None else want
    labels = torch.from_numpy(vol.reshape(-1).copy()).to(DEV)
    r = run_r(vol, value, weights)
    assert np.array_equal(r.cpu().numpy().view(np.uint32).reshape(shape), r_want)
    max_r = int(r_want.max())
    every, totals = run_centres(r, shape, weights, None)
    assert np.array_equal(np.sort(every.cpu().numpy()), tc.oracle_centres_all(vol, value))
    need = th.need_table_scaled(max_r, weights)
    centres, totals = run_centres(r, shape, weights, need)
    kept = th.centres_host(r_want, need)
    assert np.array_equal(np.sort(centres.cpu().numpy()), kept)          # the kept set equals the host's
    z, y, _ = np.unravel_index(kept, shape)
    assert totals == [len(kept), int(th._ball_rows(z.astype(np.int64), y.astype(np.int64), r_want.reshape(-1)[kept], shape, weights).sum())]
    levels, t2 = run_paint_resolve(labels, r, shape, weights, value, centres, max_r, pieces)
    assert np.array_equal(levels[0].reshape(shape), want)               # the balls lie inside the value: the painted map IS T2
    assert np.array_equal(levels, th.resolve_host(th.paint_host(r_want, kept, len(levels), weights), shape[2]))
    got = t2.cpu().numpy()
    member = vol.reshape(-1) == value
    assert np.array_equal(got.view(np.uint32)[member], want.reshape(-1)[member]) and (got[~member] == GARBAGE32).all()
    levels_all, _ = run_paint_resolve(labels, r, shape, weights, value, every, max_r, pieces)    # dropping nothing paints the same map
    assert np.array_equal(levels_all[0], levels[0])


@pytest.mark.parametrize("weights", ac.WEIGHTS)
@pytest.mark.parametrize("name", ["blobs", "touching", "debris", "long_box"])
def test_thickness_named_volumes_against_the_oracle(name, weights):
    vol = tc.VOLUMES[name]()
    for value in tc.values_of(vol):
        assert_thickness(vol, value, weights, ac.t2_cached(name, value, weights))


@pytest.mark.parametrize("x,weights", [(63, (3, 1, 1)), (64, (5, 2, 2)), (65, (1, 2, 3)), (129, (2, 1, 4))])
def test_thickness_rows_that_end_before_on_and_after_a_wave(x, weights):
    assert_thickness(tc.slab(x), 1, weights)


@pytest.mark.parametrize("shape,weights", [((1, 1, 130), (3, 1, 2)), ((7, 1, 70), (5, 2, 2)), ((1, 9, 66), (1, 2, 3))])
def test_thickness_axes_of_length_one(shape, weights):
    assert_thickness(ac.axis_one_volume(shape), 1, weights)


@pytest.mark.parametrize("weights", [(2, 1, 1), (1, 1, 2)])
def test_thickness_spans_on_every_level_and_a_list_in_pieces(weights):
    vol = tc.disc_prism()
    assert th.table_levels(80, int(ac.exact_r(vol, 1, weights).max()), weights[2] ** 2) >= 6
    assert_thickness(vol, 1, weights, pieces=3)


def test_thickness_unit_weights_through_the_scaled_entries():
    """weights (1, 1, 1): the seven-row table and the scaled kernels give what the unscaled entry points give"""
    vol = tc.blobs()
    assert_thickness(vol, 1, (1, 1, 1), tc.oracle_cached("blobs", 1))
    assert np.array_equal(ac.t2_cached("blobs", 1, (1, 1, 1)), tc.oracle_cached("blobs", 1))


# ---- the Python routes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights", [(3, 1, 1), (5, 2, 2)])
def test_thickness_device_route_equals_host_route(weights):
    spacing = [0.5 * w for w in weights]
    for name in ("touching", "debris"):
        vol = tc.VOLUMES[name]()
        settings = SimpleNamespace(voxel_spacing=spacing, thickness_save_volume=True)
        got, host = th.thickness_label_volume(torch.from_numpy(vol).to(DEV), settings), th.thickness_label_volume(vol, settings, device="cpu")
        assert np.array_equal(got["squared"], host["squared"]) and np.array_equal(got["volume"], host["volume"]) and got["settings"] == host["settings"]
        for value in tc.values_of(vol):
            assert np.array_equal(got["squared"][vol == value], ac.t2_cached(name, value, weights)[vol == value])
            a, b = got["values"][value], host["values"][value]
            assert np.array_equal(a["histogram"], b["histogram"]) and a["figures"] == b["figures"]
            assert (a["max_squared_radius"], a["centres"], a["row_spans"], a["levels"]) == (b["max_squared_radius"], b["centres"], b["row_spans"], b["levels"])


def test_the_ball_sampled_at_spacing_3_1_1():
    ball = ac.physical_ball()
    with_key = th.thickness_label_volume(ball, SimpleNamespace(voxel_spacing=[3, 1, 1]), device=DEV)
    assert with_key["values"][1]["figures"]["largest_inscribed_diameter"] == 2.0 * math.sqrt(145.0)
    assert np.array_equal(with_key["squared"], ac.oracle_t2(ball, 1, (3, 1, 1)))
    without = th.thickness_label_volume(ball, SimpleNamespace(), device=DEV)
    assert without["values"][1]["figures"]["largest_inscribed_diameter"] == 2.0 * math.sqrt(17.0)
    same = th.thickness_label_volume(ball, SimpleNamespace(voxel_spacing=[2, 2, 2]), device=DEV)       # isotropic: the unscaled kernels
    assert np.array_equal(same["squared"], without["squared"]) and same["values"][1]["histogram"].tobytes() == without["values"][1]["histogram"].tobytes()
    assert same["values"][1]["figures"]["largest_inscribed_diameter"] == 2.0 * 2.0 * math.sqrt(17.0)


def test_device_transform_route():
    seeds = tc.blobs((9, 12, 70), 11) == 0
    got = sd.squared_distance_transform(torch.from_numpy(seeds).to(DEV), spacing=[2.5, 1, 1])
    assert np.array_equal(got, ac.weighted_d2(seeds, (5, 2, 2))) and np.array_equal(got, sd.squared_distance_transform(seeds, device="cpu", spacing=[2.5, 1, 1]))
    assert np.array_equal(sd.squared_distance_transform(seeds, device=DEV, spacing=[3, 3, 3]), sd.squared_distance_transform(seeds, device=DEV))


@pytest.mark.parametrize("ignore", [False, True])
@pytest.mark.parametrize("name", sorted(ac.SPACINGS))
def test_surface_distances_device_host_and_oracles(name, ignore):
    spacing, tolerance = ac.SPACINGS[name]
    weights, unit = lv.voxel_grid(spacing)
    pred, truth, raw, ignored = ac.scored_pair()
    kw = dict(label_values=ac.LABEL_VALUES, ignore_label=255) if ignore else {}
    got, inf = sd.surface_distance_histograms(pred, raw if ignore else truth, 5, device=DEV, spacing=spacing, **kw)
    host, host_inf = sd.surface_distance_histograms(pred, raw if ignore else truth, 5, device="cpu", spacing=spacing, **kw)
    want, want_inf = ac.histograms_np(pred, truth, 5, weights, ignored if ignore else None)
    assert np.array_equal(got, want) and np.array_equal(inf, want_inf) and np.array_equal(got, host) and np.array_equal(inf, host_inf)
    scores = sd.surface_scores_from_histograms(got, inf, tolerance, unit)
    ac.assert_scores_equal(scores, ac.coordinate_scores(pred, truth, 5, spacing, tolerance, ignored if ignore else None))
    assert np.isinf(scores.hausdorff[3]) and np.isnan(scores.hausdorff[4]) and inf[3, 0] > 0 and inf[4].tolist() == [0, 0]


def test_histogram_of_a_weighted_map_takes_the_spacing():
    """a small volume whose weighted T2 lies beyond the unit-voxel bound of its shape: without the spacing the device would clamp it"""
    vol = np.zeros((3, 3, 6), np.uint8)
    vol[:, :, 1:] = 1
    t2 = th.local_thickness_squared(vol, 1, device=DEV, spacing=[1, 1, 7])
    assert np.array_equal(t2, ac.oracle_t2(vol, 1, (1, 1, 7))) and int(t2.max()) > sd.histogram_bins(vol.shape)
    want = np.bincount(t2[vol == 1].astype(np.int64))
    assert np.array_equal(th.thickness_histogram(t2, vol, 1, device=DEV, spacing=[1, 1, 7]), want)
    assert np.array_equal(th.thickness_histogram(t2, vol, 1, device="cpu", spacing=[1, 1, 7]), want)


def test_masked_maximum_sets_the_bins():
    d2 = torch.tensor([5, -1, 70000, 9, -1, 3], dtype=torch.int32, device=DEV)
    mask = torch.tensor([1, 1, 0, 1, 0, 0], dtype=torch.uint8, device=DEV)
    assert sd.masked_max_device(mask, d2) == 9 and sd.masked_max_device(torch.zeros_like(mask), d2) == 0
    high = torch.tensor([-2, 4], dtype=torch.int32, device=DEV)         # 0xFFFFFFFE: the largest finite value
    assert sd.masked_max_device(torch.ones(2, dtype=torch.uint8, device=DEV), high) == 0xFFFFFFFE


@pytest.mark.parametrize("weights", [(3, 1, 1), (5, 2, 2)])
@pytest.mark.parametrize("name", ac.PACKINGS)
def test_separation_device_equals_host_and_oracle(name, weights):
    vol = spc.scene(name)
    spacing = [0.5 * w for w in weights]
    for depth in spc.DEPTHS:
        got = sp.separate_objects(torch.from_numpy(np.asarray(vol)).to(DEV), depth=depth, spacing=spacing)
        host = sp.separate_objects(vol, depth=depth, device="cpu", spacing=spacing)
        assert got["objects"].tobytes() == host["objects"].tobytes() and got["report"] == host["report"]
        for key in host["contacts"]:
            assert np.array_equal(got["contacts"][key], host["contacts"][key]), key
        ac.assert_separation_equals_oracle(got, name, weights, depth)


@pytest.mark.parametrize("name", ["two_balls", "two_values"])
def test_isotropic_spacing_separates_as_no_spacing(name):
    vol = torch.from_numpy(np.asarray(spc.scene(name))).to(DEV)
    for depth in spc.DEPTHS:
        plain, keyed = sp.separate_objects(vol, depth=depth), sp.separate_objects(vol, depth=depth, spacing=[2, 2, 2])
        assert keyed["objects"].tobytes() == plain["objects"].tobytes() and keyed["report"] == plain["report"]
        for key in plain["contacts"]:
            assert keyed["contacts"][key].tobytes() == plain["contacts"][key].tobytes(), key


# ---- the manager -------------------------------------------------------------------------------------------------------------------
KEYS = dict(measure_objects=True, measure_separate=True, mesh_surfaces=True, thickness_map=True, thickness_save_volume=True)


def _predict(folder, labels, **keys):
    from volume_segmantics_amd.model.operations import vol_seg_prediction_manager as pm
    folder.mkdir()
    fake = SimpleNamespace(_predict_single_axis=lambda vol, axis: (labels, None), model_device_num=0, num_labels=3, label_codes={})
    settings = SimpleNamespace(one_hot=False, quality="low", prediction_axis="Z", output_probs=False, evaluation_surface_distances=True,
                               evaluation_surface_tolerance=1.3, **KEYS, **keys)
    manager = pm.VolSeg2DPredictionManager.__new__(pm.VolSeg2DPredictionManager)
    manager.predictor, manager.settings, manager.data_vol, manager.input_data_chunking, manager.downsample = fake, settings, labels, True, False
    truth = np.roll(labels, 1, axis=1)
    manager.evaluate_volume(truth, folder / "seg.h5")
    return manager, {p.name: p.read_bytes() for p in sorted(folder.iterdir())}


def _without_grid(doc):
    if isinstance(doc, dict):
        return {k: _without_grid(v) for k, v in doc.items() if k not in ("voxel_spacing", "weights", "unit")}
    return [_without_grid(v) for v in doc] if isinstance(doc, list) else doc


def test_manager_with_and_without_the_key(tmp_path):
    labels = np.ascontiguousarray(spc.scene("two_values"))
    _, plain = _predict(tmp_path / "plain", labels)
    _, again = _predict(tmp_path / "again", labels)       # two runs agree: the device route is deterministic (that the key's absence changes
    assert plain == again and {                           # nothing is held by tests/test_anisotropy_host.py against recorded bytes, and by the existing suite)"seg_thickness.json", "seg_thickness.h5", "seg_objects.json", "seg_object_contacts.json", "seg_meshes.json",
                               "seg_surface_scores.json", "seg_surface_scores.csv"} <= set(plain)
    for name, data in plain.items():
        assert b"voxel_spacing" not in data, name
    _, unit = _predict(tmp_path / "unit", labels, voxel_spacing=[1, 1, 1])
    assert sorted(unit) == sorted(plain)
    for name in plain:                                                  # a unit grid runs the same kernels: only the three fields are new
        if name.endswith(".json"):
            doc = _without_grid(json.loads(unit[name]))
            if name == "seg_object_contacts.json":
                doc.pop("neck_radius")
            assert doc == json.loads(plain[name]), name
        else:
            assert unit[name] == plain[name], name

    manager, keyed = _predict(tmp_path / "keyed", labels, voxel_spacing=[2.5, 1, 1])
    for name in ("seg_thickness.json", "seg_object_contacts.json"):
        s = json.loads(keyed[name])["settings"]
        assert (s["voxel_spacing"], s["weights"], s["unit"]) == ([2.5, 1.0, 1.0], [5, 2, 2], 0.5), name
    doc = json.loads(keyed["seg_surface_scores.json"])
    assert (doc["voxel_spacing"], doc["weights"], doc["unit"]) == ([2.5, 1.0, 1.0], [5, 2, 2], 0.5)
    assert json.loads(keyed["seg_objects.json"])["voxel_size"] == [2.5, 1.0, 1.0]              # measure and mesh default to the key
    assert manager.last_meshes["settings"]["voxel_size"] == [2.5, 1.0, 1.0]
    for value in (1, 2):
        assert np.array_equal(manager.last_thickness["squared"][labels == value], ac.oracle_t2(labels, value, (5, 2, 2))[labels == value])
    assert np.array_equal(manager.last_thickness["volume"], (2.0 * 0.5 * np.sqrt(manager.last_thickness["squared"].astype(np.float64))).astype(np.float32))
    host = sp.separate_objects(labels, device="cpu", spacing=[2.5, 1, 1])
    assert manager.last_measurements["separation"]["report"] == host["report"]
    truth = np.roll(labels, 1, axis=1)
    ac.assert_scores_equal(manager.last_evaluation["surface_scores"], ac.coordinate_scores(labels, truth, 3, [2.5, 1.0, 1.0], 1.3))

    for key in ("thickness_voxel_size", "evaluation_voxel_size"):
        with pytest.raises(ValueError, match=f"voxel_spacing and {key}"):
            _predict(tmp_path / key, labels, voxel_spacing=[2.5, 1, 1], **{key: 1.0})
