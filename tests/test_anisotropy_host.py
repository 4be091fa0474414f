"""voxel_spacing on a host: the rule that turns a spacing into integer weights, and the host routes of the distance transform, the
local thickness, the surface distances and the separation on a weighted grid against the brute-force oracle of
tests/anisotropy_cases.py - integer for integer; float figures within 1e-12 relative of distances computed from coordinates.  Then
the settings key: defaults, conflicts, what the files carry, and that nothing changes where the key is absent."""
import hashlib
import json
import math
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import anisotropy_cases as ac
import separation_cases as spc
import thickness_cases as tc
from volume_segmantics_amd.utilities import label_volume as lv
from volume_segmantics_amd.utilities import measurements as me
from volume_segmantics_amd.utilities import meshes as ms
from volume_segmantics_amd.utilities import separation as sp
from volume_segmantics_amd.utilities import surface_distance as sd
from volume_segmantics_amd.utilities import thickness as th

GOLDEN = tc.GOLDEN


# ---- the weights rule --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spacing,weights,unit", [([2.5, 1, 1], (5, 2, 2), 0.5), ([50, 8, 8], (25, 4, 4), 2.0), ([1, 0.7, 0.7], (10, 7, 7), 0.1),
                                                  ([40, 4, 4], (10, 1, 1), 4.0)])
def test_weights_of_a_spacing(spacing, weights, unit):
    got, u = lv.voxel_grid(spacing)
    assert got == weights and math.gcd(*got) == 1 and all(isinstance(w, int) for w in got)
    assert u == min(spacing) / min(weights)                            # the rule itself: u = s_min / m
    assert u == pytest.approx(unit, rel=1e-15)
    for s, w in zip(spacing, got):
        assert w * u == pytest.approx(s, rel=1e-6)


def test_weights_have_no_common_factor_and_isotropic_is_unit():
    rng = np.random.default_rng(0)
    for _ in range(200):
        w = rng.integers(1, 65, 3)
        u = float(rng.uniform(0.01, 30.0))
        got, unit = lv.voxel_grid((w * u).tolist())
        g = math.gcd(*[int(x) for x in w])
        assert got == tuple(int(x) // g for x in w) and math.gcd(*got) == 1
        assert unit == pytest.approx(u * g, rel=1e-6)
    assert lv.voxel_grid([2, 2, 2]) == ((1, 1, 1), 2.0) and lv.voxel_grid([0.37] * 3) == ((1, 1, 1), 0.37)


@pytest.mark.parametrize("bad", [[1, 1, math.pi], [1, 1, float("nan")], [1, float("inf"), 1], [0, 1, 1], [1, -2, 1], [1, 1], [1, 1, 1, 1], 2.0,
                                 [65, 1, 1], [1, 64.5, 1], [1, 1, 1.01 * 64]])
def test_spacings_that_are_refused(bad):
    with pytest.raises(ValueError, match="voxel_spacing"):
        lv.voxel_grid(bad)


def test_the_refusal_says_what_to_do():
    with pytest.raises(ValueError, match=r"voxel_spacing.*ratio of integers of at most 64.*round"):
        lv.voxel_grid([1, 1, math.pi])


def test_a_volume_whose_distances_do_not_fit_is_refused():
    assert lv.check_weights((64, 1, 1), (1024, 2, 2)) == (64, 1, 1)
    with pytest.raises(ValueError, match=r"below 2\^32 - 1 = 4294967295"):
        lv.check_weights((64, 1, 1), (1025, 1, 1))
    assert lv.check_weights((64, 64, 64), (1, 1, 1)) == (64, 64, 64)       # an axis of length 1 contributes nothing
    assert lv.check_weights((64, 1, 1), (1, 60000, 20000)) == (64, 1, 1)
    with pytest.raises(ValueError, match="2\\^32 - 1"):
        sd.squared_distance_transform(np.zeros((1025, 1, 1), np.uint8), device="cpu", spacing=[64, 1, 1])
    for bad in ((0, 1, 1), (1, 65, 1), (1, 1)):
        with pytest.raises(ValueError, match="weights"):
            lv.check_weights(bad, (4, 4, 4))


# ---- the transform -----------------------------------------------------------------------------------------------------------------
TRANSFORM_VOLUMES = {"blobs": lambda: tc.blobs() == 0, "debris": lambda: tc.debris() == 0, "touching": lambda: tc.touching() == 1,
                     "seedless": lambda: np.zeros((5, 6, 7), bool), "corner": lambda: ac.corner_seed((6, 9, 11)) != 0,
                     "row": lambda: tc.row() != 0, "plane": lambda: tc.blobs((1, 9, 66), 2) == 0}


@pytest.mark.parametrize("no_scipy", [False, True])
@pytest.mark.parametrize("name", sorted(TRANSFORM_VOLUMES))
def test_host_transform_against_the_oracle(name, no_scipy, monkeypatch):
    if no_scipy:
        monkeypatch.setitem(sys.modules, "scipy", None)                # the weighted NumPy min-plus
    seeds = TRANSFORM_VOLUMES[name]()
    for weights in ac.WEIGHTS + ((64, 1, 1),):
        got = sd.squared_distance_transform(seeds, device="cpu", spacing=[float(w) for w in weights])
        assert got.dtype == np.uint32 and np.array_equal(got, ac.weighted_d2(seeds, weights)), weights


def test_host_transform_isotropic_spacing_and_dimensions():
    seeds = tc.blobs() == 0
    plain = sd.squared_distance_transform(seeds, device="cpu")
    assert np.array_equal(sd.squared_distance_transform(seeds, device="cpu", spacing=[2, 2, 2]), plain)
    flat = seeds[3]                                                    # a 2-D array: the spacing is that of the last three axes
    assert np.array_equal(sd.squared_distance_transform(flat, device="cpu", spacing=[7, 2, 3]), ac.weighted_d2(flat[None], (7, 2, 3))[0])
    swapped = sd.squared_distance_transform(np.ascontiguousarray(seeds.transpose(2, 0, 1)), device="cpu", spacing=[3, 1, 2])
    assert np.array_equal(swapped.transpose(1, 2, 0), sd.squared_distance_transform(seeds, device="cpu", spacing=[1, 2, 3]))


# ---- thickness ---------------------------------------------------------------------------------------------------------------------
def test_the_seven_row_table_at_unit_weights_is_the_three_row_table():
    seven, three = th.need_table_scaled(3000, (1, 1, 1)), th.need_table(3000)
    assert seven.shape == (7, 3001) and seven.dtype == np.uint32
    for row, (dz, dy, dx) in enumerate([(0, 0, 1), (0, 1, 0), (0, 1, 1), (1, 0, 0), (1, 0, 1), (1, 1, 0), (1, 1, 1)]):
        assert th._subset_row(dz, dy, dx) == row and np.array_equal(seven[row], three[dz + dy + dx - 1]), row


@pytest.mark.parametrize("weights", ac.WEIGHTS)
def test_the_table_is_the_definition(weights):
    """need[row][r] by enumerating the lattice directly, for the small r where that is cheap"""
    table = th.need_table_scaled(150, weights)
    q = [w * w for w in weights]
    p = np.stack(np.meshgrid(*[np.arange(-13, 14)] * 3, indexing="ij"), -1).reshape(-1, 3)
    d = (p * p * q).sum(1)
    for row in range(7):
        on = [(row + 1) >> 2 & 1, (row + 1) >> 1 & 1, (row + 1) & 1]
        reach = d + sum(q[i] * (2 * np.abs(p[:, i]) + 1) for i in range(3) if on[i])
        for r in (1, 2, 3, 4, 5, 9, 17, 26, 50, 99, 150):
            assert table[row, r] == 1 + reach[d < r].max(), (row, r)


@pytest.mark.parametrize("weights", ac.WEIGHTS)
@pytest.mark.parametrize("name", ["blobs", "touching", "debris", "long_box"])
def test_host_thickness_against_the_oracle(name, weights):
    vol = tc.VOLUMES[name]()
    spacing = [0.5 * w for w in weights]
    for value in tc.values_of(vol):
        want = ac.t2_cached(name, value, weights)
        assert np.array_equal(th.local_thickness_squared(vol, value, device="cpu", spacing=spacing), want)
        t2 = np.zeros(vol.shape, np.uint32)
        th._value_host(vol, value, t2, None, prune=False, weights=weights)          # dropping nothing paints the same map
        assert np.array_equal(t2, want)


def test_pruning_drops_most_voxels_and_no_ball():
    vol = tc.disc_prism()
    for weights in ((2, 1, 1), (1, 1, 2)):
        r = ac.exact_r(vol, 1, weights)
        kept = th.centres_host(r, th.need_table_scaled(int(r.max()), weights))
        assert 0 < len(kept) < 0.5 * (vol == 1).sum()
        levels = th.table_levels(vol.shape[2], int(r.max()), weights[2] ** 2)
        every = np.flatnonzero(r.reshape(-1) > 0)
        a = th.resolve_host(th.paint_host(r, kept, levels, weights), vol.shape[2])[0]
        b = th.resolve_host(th.paint_host(r, every, levels, weights), vol.shape[2])[0]
        assert np.array_equal(a, b)


def test_the_ball_sampled_at_spacing_3_1_1():
    ball = ac.physical_ball()
    assert ball.shape == (13, 31, 31) and int(ball.sum()) == 2353
    with_key = th.thickness_label_volume(ball, SimpleNamespace(voxel_spacing=[3, 1, 1]), device="cpu")
    assert with_key["values"][1]["figures"]["largest_inscribed_diameter"] == 2.0 * math.sqrt(145.0)
    assert with_key["settings"]["weights"] == [3, 1, 1] and with_key["settings"]["unit"] == 1.0 and with_key["settings"]["voxel_spacing"] == [3.0, 1.0, 1.0]
    without = th.thickness_label_volume(ball, SimpleNamespace(), device="cpu")
    assert without["values"][1]["figures"]["largest_inscribed_diameter"] == 2.0 * math.sqrt(17.0)
    assert "weights" not in without["settings"]


def test_histogram_of_a_weighted_map_takes_the_spacing():
    """T2 under (1, 1, 7) exceeds the unit-voxel bound of the shape: the public histogram counts it with the spacing it came from"""
    vol = np.zeros((3, 3, 6), np.uint8)
    vol[:, :, 1:] = 1
    t2 = th.local_thickness_squared(vol, 1, device="cpu", spacing=[1, 1, 7])
    assert int(t2.max()) == 49 * 25 > sd.histogram_bins(vol.shape)
    hist = th.thickness_histogram(t2, vol, 1, device="cpu", spacing=[1, 1, 7])
    assert np.array_equal(hist, np.bincount(t2[vol == 1].astype(np.int64)))


def test_only_the_last_weighted_table_is_kept():
    th.need_table_scaled(100, (3, 1, 1))
    th.need_table_scaled(100, (5, 2, 2))
    assert th._need_cache["weighted"][0] == (5, 2, 2) and not any(isinstance(k, tuple) for k in th._need_cache)
    assert np.array_equal(th.need_table_scaled(100, (3, 1, 1)), th.need_table_scaled(150, (3, 1, 1))[:, :101])


def test_a_plate_reads_its_width_in_the_units_of_its_axis():
    """w voxels along an axis of step s read w s or (w + 1) s: distances run between voxel centres"""
    vol = np.zeros((16, 20, 20), np.uint8)
    vol[4:10] = 1                                                       # 6 voxels along z
    t = th.thickness_label_volume(vol, SimpleNamespace(voxel_spacing=[2.5, 1, 1]), device="cpu")
    assert t["values"][1]["figures"]["max"] == 6 * 2.5
    vol = np.zeros((16, 20, 20), np.uint8)
    vol[:, :, 4:9] = 1                                                  # 5 voxels along x
    t = th.thickness_label_volume(vol, SimpleNamespace(voxel_spacing=[2.5, 1, 1]), device="cpu")
    assert t["values"][1]["figures"]["max"] == 6 * 1.0


# ---- surface distances -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ignore", [False, True])
@pytest.mark.parametrize("name", sorted(ac.SPACINGS))
def test_host_surface_distances_against_both_oracles(name, ignore):
    spacing, tolerance = ac.SPACINGS[name]
    weights, unit = lv.voxel_grid(spacing)
    pred, truth, raw, ignored = ac.scored_pair()
    kw = dict(label_values=ac.LABEL_VALUES, ignore_label=255) if ignore else {}
    hists, inf = sd.surface_distance_histograms(pred, raw if ignore else truth, 5, device="cpu", spacing=spacing, **kw)
    want, want_inf = ac.histograms_np(pred, truth, 5, weights, ignored if ignore else None)
    assert np.array_equal(hists, want) and np.array_equal(inf, want_inf)
    scores = sd.surface_scores_from_histograms(hists, inf, tolerance, unit)
    ac.assert_scores_equal(scores, ac.coordinate_scores(pred, truth, 5, spacing, tolerance, ignored if ignore else None))
    assert np.isinf(scores.hausdorff[3]) and np.isnan(scores.hausdorff[4]) and np.isfinite(scores.hausdorff[:3]).all()


def test_a_histogram_that_would_be_too_long_is_refused():
    assert sd.bins_present((1 << 28) - 2) == 1 << 28
    with pytest.raises(ValueError, match=str((1 << 28) + 1)):
        sd.bins_present((1 << 28) - 1)


# ---- separation --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["two_balls", "three_balls", "two_values", "rows_65"])
def test_isotropic_spacing_separates_as_no_spacing(name):
    vol = spc.scene(name)
    for depth in spc.DEPTHS:
        plain = sp.separate_objects(vol, depth=depth, device="cpu")
        keyed = sp.separate_objects(vol, depth=depth, device="cpu", spacing=[2, 2, 2])
        assert keyed["objects"].tobytes() == plain["objects"].tobytes() and keyed["report"] == plain["report"]
        for key in plain["contacts"]:
            assert np.array_equal(keyed["contacts"][key], plain["contacts"][key]), key
        # the same grid with a common factor left in the weights: every R four times as large, the depth still in voxels
        doubled = sp.separate_prepared(np.asarray(vol), vol.shape, None, None, 6, depth, None, (2, 2, 2))
        assert np.array_equal(doubled[0].reshape(vol.shape), plain["objects"]) and doubled[1] == plain["report"]
        assert np.array_equal(doubled[2]["neck_squared"], 4 * plain["contacts"]["neck_squared"])


@pytest.mark.parametrize("weights", [(3, 1, 1), (5, 2, 2)])
@pytest.mark.parametrize("name", ac.PACKINGS)
def test_host_separation_against_the_oracle(name, weights):
    vol = spc.scene(name)
    for depth in spc.DEPTHS:
        got = sp.separate_objects(vol, depth=depth, device="cpu", spacing=[0.5 * w for w in weights])
        ac.assert_separation_equals_oracle(got, name, weights, depth)


def test_coarse_axes_change_what_is_one_object():
    """two balls of radius 8 voxels, centres 12 voxels apart along x: with z and y twice as coarse as x the balls are discs that
    overlap deeply, and the default depth no longer takes them apart"""
    vol = spc.scene("two_balls")
    assert sp.separate_objects(vol, device="cpu")["report"]["1"]["objects"] == 2
    got = sp.separate_objects(vol, device="cpu", spacing=[2, 2, 1])
    ac.assert_separation_equals_oracle(got, "two_balls", (2, 2, 1), sp.DEFAULT_DEPTH)
    assert got["report"]["1"]["separated"] and got["report"]["1"]["objects"] == 1


# ---- the settings key --------------------------------------------------------------------------------------------------------------
def test_the_key_is_the_default_of_measure_and_mesh_and_conflicts_with_the_scalars():
    s = SimpleNamespace(voxel_spacing=[2.5, 1, 1])
    assert me.measurement_settings(s)["voxel_size"] == [2.5, 1.0, 1.0] and ms.mesh_settings(s)["voxel_size"] == [2.5, 1.0, 1.0]
    assert me.measurement_settings(SimpleNamespace(voxel_spacing=[2.5, 1, 1], measure_voxel_size=3.0))["voxel_size"] == [3.0, 3.0, 3.0]
    both = SimpleNamespace(voxel_spacing=[2.5, 1, 1], measure_voxel_size=3.0, mesh_voxel_size=[4, 2, 2])
    assert ms.mesh_settings(both)["voxel_size"] == [4.0, 2.0, 2.0]
    assert ms.mesh_settings(SimpleNamespace(voxel_spacing=[2.5, 1, 1], measure_voxel_size=3.0))["voxel_size"] == [3.0, 3.0, 3.0]
    assert me.measurement_settings(SimpleNamespace())["voxel_size"] == [1.0, 1.0, 1.0]
    with pytest.raises(ValueError, match=r"voxel_spacing.*thickness_voxel_size|thickness_voxel_size.*voxel_spacing"):
        th.thickness_settings(SimpleNamespace(voxel_spacing=[2.5, 1, 1], thickness_voxel_size=1.0))
    with pytest.raises(ValueError, match=r"voxel_spacing.*evaluation_voxel_size|evaluation_voxel_size.*voxel_spacing"):
        sd.surface_settings(SimpleNamespace(voxel_spacing=[2.5, 1, 1], evaluation_voxel_size=1.0))
    for settings in (th.thickness_settings, sd.surface_settings, me.measurement_settings, ms.mesh_settings, sp.separation_settings):
        with pytest.raises(ValueError, match="voxel_spacing"):
            settings(SimpleNamespace(voxel_spacing=[1, 1, math.pi]))
    t = th.thickness_settings(SimpleNamespace(voxel_spacing=[2.5, 1, 1], measure_voxel_size=7.0))
    assert t["voxel_size"] == 0.5 and t["weights"] == [5, 2, 2] and t["unit"] == 0.5 and t["voxel_spacing"] == [2.5, 1.0, 1.0]
    assert sd.surface_settings(SimpleNamespace(voxel_spacing=[2.5, 1, 1], evaluation_surface_tolerance=1.3)) == (False, 1.3, 0.5)
    assert sp.separation_settings(SimpleNamespace(voxel_spacing=[3, 1, 1]))["weights"] == [3, 1, 1]
    assert "weights" not in sp.separation_settings(SimpleNamespace()) and "weights" not in th.thickness_settings(SimpleNamespace())


def _write_all(folder, settings, device="cpu"):
    """every file the analyses of a label volume write with these settings, as {name: bytes}"""
    folder.mkdir()
    vol = spc.scene("two_values")
    kept = th.thickness_label_volume(vol, settings, device=device)
    th.write_thickness(folder / "seg", kept)
    np.save(folder / "seg_thickness.npy", kept["volume"])
    m = me.measure_label_volume(vol, settings, device=device)
    me.write_measurements(folder / "seg", m["raw"], m["table"], m["settings"], m.get("separation"))
    pred, truth, raw, _ = ac.scored_pair()
    sd.evaluate_surface_distances(pred, raw, 5, settings, label_values=ac.LABEL_VALUES, ignore_label=255, device=device, stem=folder / "seg")
    return {p.name: p.read_bytes() for p in sorted(folder.iterdir())}


BASE_KEYS = dict(thickness_save_volume=True, measure_objects=True, measure_separate=True, evaluation_surface_tolerance=1.3)


def _without_grid(doc):
    if isinstance(doc, dict):
        return {k: _without_grid(v) for k, v in doc.items() if k not in ("voxel_spacing", "weights", "unit")}
    return [_without_grid(v) for v in doc] if isinstance(doc, list) else doc


def test_files_with_and_without_the_key(tmp_path):
    plain = _write_all(tmp_path / "plain", SimpleNamespace(**BASE_KEYS))
    # with the key absent every file holds the bytes that the code of the commit before the key existed wrote for the same call:
    # tests/golden/anisotropy_key_absent.json records their hashes, written by that commit's utilities (host route)
    recorded = json.loads((GOLDEN / "anisotropy_key_absent.json").read_text())["sha256"]
    assert {name: hashlib.sha256(data).hexdigest() for name, data in plain.items()} == recorded and len(plain) == 9
    for name, data in plain.items():                                   # with the key absent no file names it
        assert b"voxel_spacing" not in data and b"weights" not in data, name
    unit = _write_all(tmp_path / "unit", SimpleNamespace(voxel_spacing=[1, 1, 1], **BASE_KEYS))
    assert sorted(unit) == sorted(plain)
    for name in plain:                                                 # a unit grid: the same figures; only the three fields are new
        if name.endswith(".json"):
            doc = _without_grid(json.loads(unit[name]))
            if name == "seg_object_contacts.json":
                doc.pop("neck_radius")                                  # the sentence on the unit of the column
            assert doc == json.loads(plain[name]), name
        else:
            assert unit[name] == plain[name], name
    keyed = _write_all(tmp_path / "keyed", SimpleNamespace(voxel_spacing=[2.5, 1, 1], **BASE_KEYS))
    for name in ("seg_thickness.json", "seg_object_contacts.json"):
        s = json.loads(keyed[name])["settings"]
        assert (s["voxel_spacing"], s["weights"], s["unit"]) == ([2.5, 1.0, 1.0], [5, 2, 2], 0.5), name
    doc = json.loads(keyed["seg_objects.json"])
    assert doc["voxel_size"] == [2.5, 1.0, 1.0] and doc["separation"]["settings"]["weights"] == [5, 2, 2]
    doc = json.loads(keyed["seg_surface_scores.json"])
    assert (doc["voxel_spacing"], doc["weights"], doc["unit"], doc["voxel_size"]) == ([2.5, 1.0, 1.0], [5, 2, 2], 0.5, 0.5)
    assert keyed["seg_surface_scores.csv"].split(b"\n")[0] == plain["seg_surface_scores.csv"].split(b"\n")[0]      # the columns are unchanged
    contacts = json.loads(keyed["seg_object_contacts.json"])
    at = {c: i for i, c in enumerate(contacts["columns"])}
    assert contacts["contacts"] and "unit * sqrt(neck_squared)" in contacts["neck_radius"]
    for row in contacts["contacts"]:
        assert row[at["neck_radius"]] == 0.5 * math.sqrt(row[at["neck_squared"]])
    thick = json.loads(keyed["seg_thickness.json"])
    vol = spc.scene("two_values")
    for value in (1, 2):
        hist = thick["values"][str(value)]["histogram"]
        want = np.bincount(ac.oracle_t2(vol, value, (5, 2, 2))[vol == value].astype(np.int64))
        assert hist["squared_thickness"] == np.flatnonzero(want).tolist() and hist["count"] == want[want > 0].tolist()
        assert thick["values"][str(value)]["max"] == 2.0 * 0.5 * math.sqrt(float(hist["squared_thickness"][-1]))
