"""The host side of utilities/measurements.py (no GPU): the host route integer for integer against the per-component oracle of
tests/measurement_cases.py, closed forms of boxes, the exact covariance far from the origin, the overflow check, the selection of
rows, object ids, the settings keys, the writers, the measure command and the committed vessels integers.  Nothing has a tolerance
but the closed forms of the derived floats (np.isclose)."""
import csv
import json
import math
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import components_cases as cc
import measurement_cases as mc
from volume_segmantics_amd.utilities import measurements as me

REPO = Path(__file__).resolve().parent.parent


def host(vol, **kw):
    return me.measure_components(vol, device="cpu", **kw)


# ---- the integers ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", mc.DEGENERATE_SHAPES + [(9, 10, 67)])
def test_host_route_against_the_oracle(shape):
    for k, seed in ((2, 1), (4, 2)):
        vol = cc.random_labels(shape, k, 0.5, seed)
        for c in cc.CONNECTIVITIES:
            mc.assert_raw_equal(host(vol, connectivity=c), mc.oracle_measure(vol, c), (shape, k, c))
            mc.assert_raw_equal(host(vol, connectivity=c, include_background=True, min_voxels=3),
                                mc.oracle_measure(vol, c, min_voxels=3, include_background=True), (shape, k, c, "background"))


def test_oracle_agrees_with_scipy():
    vol = cc.random_labels((9, 10, 67), 4, 0.5, 2)
    comp = cc.oracle_roots(vol, 18)
    raw = mc.oracle_measure(vol, 18, include_background=True, roots=comp)
    mc.scipy_cross_check(vol, comp, raw)
    assert raw["table"][:, 0].sum() == vol.size
    for axis in range(3):                                           # every face between two values is exposed once from each side
        differing = int((np.diff(vol.astype(np.int16), axis=axis) != 0).sum())
        outer = 2 * vol.size // vol.shape[axis]
        assert raw["table"][:, 16 + axis].sum() == 2 * differing + outer


def test_box_closed_forms():
    a, b, c = 2, 3, 4
    vol = mc.box_in_volume((12, 14, 20), (3, 4, 5), (a, b, c))
    raw = host(vol)
    assert raw["table"].shape == (1, 20) and raw["roots"].tolist() == [np.ravel_multi_index((3, 4, 5), vol.shape)] and raw["values"].tolist() == [1]
    row = dict(zip(me.FIELDS, raw["table"][0].tolist()))
    assert row["voxels"] == a * b * c
    assert [row["faces_z"], row["faces_y"], row["faces_x"]] == [2 * b * c, 2 * a * c, 2 * a * b] == [24, 16, 12]
    assert [row["min_z"], row["max_z"], row["min_y"], row["max_y"], row["min_x"], row["max_x"]] == [3, 4, 4, 6, 5, 8] and row["touches_border"] == 0
    assert raw["not_listed_objects"][0] == 1 and raw["not_listed_voxels"][0] == vol.size - a * b * c

    size = (3.0, 0.5, 2.0)
    o = me.object_table(raw, voxel_size=size)["objects"]
    assert o["volume"][0] == a * b * c * 3.0 and [o["centroid_z"][0], o["centroid_y"][0], o["centroid_x"][0]] == [3.5, 5.0, 6.5]
    assert [o["extent_z"][0], o["extent_y"][0], o["extent_x"][0]] == [a, b, c]
    area = 2 * b * c * 0.5 * 2.0 + 2 * a * c * 3.0 * 2.0 + 2 * a * b * 3.0 * 0.5
    assert np.isclose(o["surface_area"][0], area)
    assert np.isclose(o["sphericity"][0], math.pi ** (1 / 3) * (6 * a * b * c * 3.0) ** (2 / 3) / area)
    assert np.isclose(o["equivalent_diameter"][0], (6 * a * b * c * 3.0 / math.pi) ** (1 / 3))
    # variances (extent^2 - 1) / 12 in voxels, scaled by the voxel size; the box is aligned, so these are the eigenvalues
    want = sorted((math.sqrt((e * e - 1) / 12.0) * s for e, s in zip((a, b, c), size)), reverse=True)
    assert np.allclose([o["axis_1"][0], o["axis_2"][0], o["axis_3"][0]], want)
    assert np.isclose(o["elongation"][0], want[1] / want[0]) and np.isclose(o["flatness"][0], want[2] / want[1])
    cube = me.object_table(host(mc.box_in_volume((9, 9, 9), (2, 2, 2), (4, 4, 4))))["objects"]
    assert np.isclose(cube["sphericity"][0], (math.pi / 6) ** (1 / 3)) and np.isclose(cube["elongation"][0], 1.0)


def test_two_boxes_meeting_at_a_corner():
    vol = np.zeros((8, 8, 8), dtype=np.uint8)
    vol[1:3, 1:3, 1:3] = 1
    vol[3:6, 3:6, 3:6] = 1
    assert host(vol, connectivity=6)["table"][:, 0].tolist() == [8, 27] and host(vol, connectivity=18)["table"][:, 0].tolist() == [8, 27]
    joined = host(vol, connectivity=26)
    assert joined["table"][:, 0].tolist() == [35] and joined["table"][0, 16:19].tolist() == [2 * (4 + 9)] * 3
    assert joined["table"][0, 10:16].tolist() == [1, 5, 1, 5, 1, 5]


def test_box_on_the_boundary_counts_its_outward_faces():
    vol = mc.box_in_volume((6, 7, 8), (0, 2, 5), (2, 3, 3), value=9)        # against z = 0 and x = 7
    raw = host(vol)
    assert raw["table"][0, 16:19].tolist() == [2 * 3 * 3, 2 * 2 * 3, 2 * 2 * 3] and raw["table"][0, 19] == 1
    assert me.object_table(raw)["objects"]["touches_border"].tolist() == [1]
    flat = host(mc.box_in_volume((1, 7, 8), (0, 2, 2), (1, 3, 3)))           # z of length 1: no faces across it, and it is no boundary
    assert flat["table"][0, 16:20].tolist() == [0, 6, 6, 0]


def test_far_object_keeps_its_covariance():
    """a 2 x 3 x 3 box 60 000 voxels along x: mean x^2 is 3.6e9 and the variance 2 / 3 - mean(x^2) - mean(x)^2 in float64 keeps seven digits
    of it; the exact numerator n sum x^2 - (sum x)^2 is the same integer wherever the box sits"""
    vol = np.zeros((3, 4, 60010), dtype=np.uint8)
    vol[0:2, 0:3, 60000:60003] = 1
    near = np.zeros((3, 4, 12), dtype=np.uint8)
    near[0:2, 0:3, 2:5] = 1
    raw = host(vol)
    far_o, near_o = me.object_table(raw)["objects"], me.object_table(host(near))["objects"]
    for name in ("axis_1", "axis_2", "axis_3", "elongation", "flatness"):
        assert far_o[name][0] == near_o[name][0], name                # bit for bit
    assert np.isclose(far_o["axis_1"][0], math.sqrt(8 / 12)) and np.isclose(far_o["axis_3"][0], 0.5) and far_o["centroid_x"][0] == 60001.0
    t = raw["table"][0].astype(np.float64)
    assert not np.isclose(t[6] / t[0] - (t[3] / t[0]) ** 2, 8 / 12, rtol=1e-9, atol=0)      # the float difference it replaces is wrong here


def test_sums_that_do_not_fit_are_refused():
    big = np.broadcast_to(np.zeros((), np.uint8), (1, 30000, 70000))         # a view: no memory behind it
    assert big.size < 2 ** 31 and big.size * 69999 ** 2 >= 2 ** 63
    with pytest.raises(ValueError, match="does not fit int64"):
        me.measure_components(big, device="cpu")
    with pytest.raises(ValueError, match="does not fit int64"):
        me.object_ids(big, device="cpu")
    me._check_sums_fit((1024, 1024, 2047))                            # the largest cube-like volumes pass


def test_min_voxels_background_and_not_listed_totals():
    vol = cc.cleanup_scene()
    everything = host(vol, include_background=True)
    sizes = {v: sorted(everything["table"][everything["values"] == v, 0].tolist()) for v in range(4)}
    assert sum(map(sum, sizes.values())) == vol.size and not everything["not_listed_objects"].any()
    some = host(vol, min_voxels=27)
    for v in range(1, 4):
        kept = [s for s in sizes[v] if s >= 27]
        assert sorted(some["table"][some["values"] == v, 0].tolist()) == kept
        assert some["not_listed_objects"][v] == len(sizes[v]) - len(kept) and some["not_listed_voxels"][v] == sum(sizes[v]) - sum(kept)
    assert 0 not in some["values"] and some["not_listed_objects"][0] == len(sizes[0]) and some["not_listed_voxels"][0] == sum(sizes[0])
    mc.assert_raw_equal(some, mc.oracle_measure(vol, 6, min_voxels=27))
    other = host(vol, background=1, min_voxels=5)                     # another background value
    assert 1 not in other["values"] and 0 in other["values"]
    summary = me.object_table(some)["summary"]
    assert summary["3"] == dict(objects=0, voxels=0, volume=0.0, volume_fraction=0.0, largest_object=0, median_object=summary["3"]["median_object"],
                                not_listed_objects=1, not_listed_voxels=cc.SCENE["object_3"]) and math.isnan(summary["3"]["median_object"])
    assert summary["2"]["objects"] == 2 and summary["2"]["largest_object"] == 27 and summary["2"]["median_object"] == 27.0
    assert summary["2"]["volume_fraction"] == 54 / vol.size and summary["2"]["not_listed_voxels"] == cc.SCENE["bar"]
    with pytest.raises(ValueError, match="min_voxels"):
        host(vol, min_voxels=0)
    with pytest.raises(ValueError, match="connectivity 7"):
        host(vol, connectivity=7)


def test_row_order_ids_and_object_ids():
    vol = np.array([0, 7, 100, 200], dtype=np.uint8)[cc.cleanup_scene()]
    raw = host(vol, connectivity=18)
    order = list(zip(raw["values"].tolist(), raw["roots"].tolist()))
    assert order == sorted(order) and len(set(raw["values"].tolist())) == 3
    table = me.object_table(raw)["objects"]
    assert table["id"].tolist() == list(range(1, len(order) + 1)) and np.array_equal(table["root"], raw["roots"])
    assert np.array_equal(np.ravel_multi_index((table["root_z"], table["root_y"], table["root_x"]), vol.shape), raw["roots"])
    ids = me.object_ids(vol, connectivity=18, device="cpu")
    assert ids.dtype == np.int32 and ids.shape == vol.shape and (ids[vol == 0] == 0).all() and (ids[vol != 0] > 0).all()
    assert np.array_equal(np.bincount(ids.reshape(-1))[1:], raw["table"][:, 0])
    assert np.array_equal(ids.reshape(-1)[raw["roots"]], table["id"])
    few = me.object_ids(vol, min_voxels=27, device="cpu")
    assert np.array_equal(np.bincount(few.reshape(-1))[1:], host(vol, min_voxels=27)["table"][:, 0])
    plane = me.object_ids(vol[5], device="cpu")                      # a 2-D volume keeps its shape
    assert plane.shape == vol[5].shape


# ---- settings, writers, command ----------------------------------------------------------------------------------------------------
def test_settings_defaults_and_parsing():
    assert me.measurement_settings(SimpleNamespace()) == dict(active=False, connectivity=6, min_voxels=1, include_background=False,
                                                              voxel_size=[1.0, 1.0, 1.0], save_ids=False)
    assert me.measurement_settings(SimpleNamespace(postprocess_connectivity=26))["connectivity"] == 26
    assert me.measurement_settings(SimpleNamespace(postprocess_connectivity=26, measure_connectivity=18))["connectivity"] == 18
    on = me.measurement_settings(SimpleNamespace(measure_objects=True, measure_min_voxels=64, measure_background=True, measure_voxel_size=[2, 0.5, 1],
                                                 measure_save_ids=True))
    assert on == dict(active=True, connectivity=6, min_voxels=64, include_background=True, voxel_size=[2.0, 0.5, 1.0], save_ids=True)
    assert me.measurement_settings(SimpleNamespace(measure_voxel_size=0.25))["voxel_size"] == [0.25] * 3
    for bad in (dict(measure_connectivity=8), dict(measure_min_voxels=0), dict(measure_voxel_size=[1, 2]), dict(measure_voxel_size=-1.0)):
        with pytest.raises(ValueError):
            me.measurement_settings(SimpleNamespace(**bad))
    shipped = (REPO / "volseg-settings" / "2d_model_predict_settings.yaml").read_text()
    for key in ("measure_objects", "measure_connectivity", "measure_min_voxels", "measure_background", "measure_voxel_size", "measure_save_ids"):
        assert f"# {key}:" in shipped                                # documented, commented out: the shipped settings measure nothing
    from volume_segmantics_amd.data import get_settings_data
    assert not me.measurement_settings(get_settings_data(REPO / "volseg-settings" / "2d_model_predict_settings.yaml"))["active"]


def test_manager_keys_are_absent_safe(tmp_path, monkeypatch):
    """a settings object without the keys: inactive, the manager's measuring branch is not entered and no _objects file appears"""
    from volume_segmantics_amd.model.operations import vol_seg_prediction_manager as pm
    from volume_segmantics_amd.utilities import base_data_utils as utils
    assert me.measurement_settings(SimpleNamespace(one_hot=False))["active"] is False
    labels = cc.random_labels((4, 5, 6), 3, 0.5, 1)
    fake = SimpleNamespace(_predict_single_axis=lambda vol, axis: (labels, None), model_device_num=0)
    settings = SimpleNamespace(one_hot=False, quality="low", prediction_axis="Z", output_probs=False)
    manager = pm.VolSeg2DPredictionManager.__new__(pm.VolSeg2DPredictionManager)
    manager.predictor, manager.settings, manager.data_vol, manager.input_data_chunking = fake, settings, labels, True
    monkeypatch.setattr(me, "measure_label_volume", lambda *a, **k: pytest.fail("measured without the key"))
    out = manager.predict_volume_to_path(tmp_path / "seg.h5")
    assert np.array_equal(out, labels) and manager.last_measurements is None
    assert [p.name for p in tmp_path.iterdir()] == ["seg.h5"] and np.array_equal(utils.numpy_from_hdf5(tmp_path / "seg.h5")[0], labels)
    settings.measure_objects = False
    manager.predict_volume_to_path(tmp_path / "seg.h5")
    assert [p.name for p in tmp_path.iterdir()] == ["seg.h5"]
    settings.measure_objects, settings.one_hot = True, True
    with pytest.raises(ValueError, match="one_hot"):
        manager.predict_volume_to_path(None)


def test_writers_round_trip_and_nan_as_null(tmp_path):
    vol = cc.cleanup_scene().copy()
    vol[38, 46, 70] = 3                                              # a single voxel: no axes, elongation and flatness are NaN
    m = me.measure_label_volume(vol, SimpleNamespace(measure_min_voxels=1, measure_voxel_size=[2.0, 1.0, 0.5], measure_connectivity=18), device="cpu")
    assert m["ids"] is None and m["settings"]["connectivity"] == 18
    written = me.write_measurements(tmp_path / "seg", m["raw"], m["table"], m["settings"])
    assert [p.name for p in written] == ["seg_objects.csv", "seg_objects.json"]
    text = written[1].read_text()
    assert "NaN" not in text and "null" in text
    doc = json.loads(text)
    assert doc["settings"] == m["settings"] and doc["fields"] == list(me.FIELDS) and doc["shape"] == list(vol.shape)
    back = me.raw_from_json(doc)
    assert np.array_equal(back["table"], m["raw"]["table"]) and np.array_equal(back["roots"], m["raw"]["roots"])
    again = me.object_table(back, doc["voxel_size"])                 # reproducible to the bit from the file's integers
    for name in me.COLUMNS:
        assert np.array_equal(again["objects"][name], m["table"]["objects"][name], equal_nan=True), name
    assert again["summary"].keys() == m["table"]["summary"].keys()
    single = [o for o in doc["objects"] if o["raw"][0] == 1]
    assert len(single) == 1 and all(o["derived"]["elongation"] is None and o["derived"]["flatness"] is None for o in single)
    with open(written[0], newline="") as f:
        rows = list(csv.reader(f))
    assert tuple(rows[0]) == me.COLUMNS and len(rows) == 1 + len(doc["objects"])
    first = dict(zip(rows[0], rows[1]))
    assert int(first["voxels"]) == doc["objects"][0]["raw"][0] and float(first["volume"]) == m["table"]["objects"]["volume"][0]
    assert "largest objects" in me.object_table_text(m["table"]) and me.object_table_text(m["table"]).count("\n") >= 12


def test_measure_command_on_an_hdf5_file(tmp_path):
    """the file is written and read through base_data_utils: h5py where it is installed, hdf5_lite where it is not"""
    from volume_segmantics_amd.scripts import measure_2d_prediction
    from volume_segmantics_amd.utilities import arg_parsing
    from volume_segmantics_amd.utilities import base_data_utils as utils
    vol = np.array([0, 7, 100, 200], dtype=np.uint8)[cc.cleanup_scene()]
    (tmp_path / "volseg-settings").mkdir()
    (tmp_path / "volseg-settings" / "2d_model_predict_settings.yaml").write_text(
        "measure_min_voxels: 5\nmeasure_voxel_size: [2.0, 1.0, 1.0]\nmeasure_save_ids: true\npostprocess_connectivity: 26\n")      # no measure_objects: the command is the request
    utils.save_data_to_hdf5(vol, tmp_path / "pred.h5")
    measure_2d_prediction.main([str(tmp_path / "pred.h5"), "--data_dir", str(tmp_path)])
    assert {p.name for p in tmp_path.iterdir()} == {"volseg-settings", "pred.h5", "pred_objects.csv", "pred_objects.json", "pred_object_ids.h5"}
    doc = json.loads((tmp_path / "pred_objects.json").read_text())
    want = mc.oracle_measure(vol, 26, min_voxels=5)
    assert doc["settings"]["connectivity"] == 26 and doc["voxel_size"] == [2.0, 1.0, 1.0]
    mc.assert_raw_equal(dict(me.raw_from_json(doc)), want)
    ids = utils.numpy_from_hdf5(tmp_path / "pred_object_ids.h5")[0]
    assert np.array_equal(ids, me.object_ids(vol, connectivity=26, min_voxels=5, device="cpu"))
    measure_2d_prediction.main([str(tmp_path / "pred.h5"), "--data_dir", str(tmp_path), "--output", str(tmp_path / "other")])
    assert (tmp_path / "other_objects.json").read_text() == (tmp_path / "pred_objects.json").read_text()
    for bad in ([str(tmp_path / "missing.h5")], [str(tmp_path / "pred.h5"), "--output", str(tmp_path / "nowhere" / "stem")], []):
        with pytest.raises(SystemExit) as stop:
            arg_parsing.parse_measuring_args(bad)
        assert stop.value.code == 2


@pytest.mark.parametrize("connectivity", [6, 26])
def test_vessels_fixture_against_the_committed_integers(connectivity):
    expected = mc.vessels_expected()[str(connectivity)]
    raw = host(cc.vessels(), connectivity=connectivity, include_background=True)
    assert raw["roots"].tolist() == expected["roots"] and raw["values"].tolist() == expected["values"]
    assert raw["table"].tolist() == expected["table"]
    assert {str(v): [int(raw["not_listed_objects"][v]), int(raw["not_listed_voxels"][v])] for v in np.flatnonzero(raw["not_listed_objects"])} == expected["not_listed"]
