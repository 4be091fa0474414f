"""Local thickness on a host (utilities/thickness.py, device="cpu"): T2 array for array against the brute-force oracle of
tests/thickness_cases.py on every named volume, the oracle against the scipy formulation, the containment table against its
definition, pruning against no pruning, the figures against NumPy on the expanded thicknesses, the stated bias, the settings, the
files, the committed vessels figures, the command and the manager.  Integers have no tolerance; the float64 figures get 1e-12."""
import csv
import json
import math
from types import SimpleNamespace

import numpy as np
import pytest

import thickness_cases as tc
from volume_segmantics_amd.utilities import thickness as th

REPO = tc.GOLDEN.parent.parent


def host(vol, value, **kw):
    return th.local_thickness_squared(vol, value, device="cpu", **kw)


# ---- T2 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(tc.VOLUMES))
def test_host_route_equals_the_oracle(name):
    vol = tc.VOLUMES[name]()
    for value in tc.values_of(vol):
        want = tc.oracle_cached(name, value)
        got = host(vol, value)
        assert got.dtype == np.uint32 and got.shape == vol.shape and np.array_equal(got, want), (name, value)
        assert not got[vol != value].any()
        r = tc.exact_r(vol, value)
        if r is not None:
            assert (got.astype(np.int64) >= r).all() and got.max() == r.max()


@pytest.mark.parametrize("name", sorted(set(tc.VOLUMES) - {"vessels_crop"}))
def test_oracle_equals_the_scipy_formulation(name):
    vol = tc.VOLUMES[name]()
    for value in tc.values_of(vol):
        other = tc.scipy_t2(vol, value)
        if other is None:                                                # scipy does not import: there is no second formulation to hold
            return
        assert np.array_equal(other, tc.oracle_cached(name, value)), (name, value)


def test_value_without_another_value_has_no_thickness():
    vol = tc.filled()
    assert not host(vol, 3).any() and not host(vol, 1).any()
    t = th.thickness_label_volume(vol, SimpleNamespace(), device="cpu")
    row = t["values"][3]
    assert row["figures"]["voxels"] == vol.size and all(math.isnan(row["figures"][name]) for name in th.FIGURES)
    assert row["max_squared_radius"] is None and row["centres"] == 0 and not t["squared"].any()


def test_several_values_share_one_map():
    vol = tc.touching()
    t = th.thickness_label_volume(vol, SimpleNamespace(thickness_values=[0, 1, 2]), device="cpu")
    want = sum(tc.oracle_t2(vol, value).astype(np.int64) for value in (0, 1, 2))       # the values' maps are disjoint
    assert np.array_equal(t["squared"], want) and list(t["values"]) == [0, 1, 2]
    only = th.thickness_label_volume(vol, SimpleNamespace(thickness_values=[2]), device="cpu")["squared"]
    assert np.array_equal(only, tc.oracle_cached("touching", 2)) and not only[vol != 2].any()


def test_one_and_two_dimensional_arrays_keep_their_shape():
    vol = tc.row()
    assert np.array_equal(host(vol[0, 0], 1), tc.oracle_cached("row", 1)[0, 0])
    flat = tc.VOLUMES["blobs_2d"]()
    assert np.array_equal(host(flat[0], 1), tc.oracle_cached("blobs_2d", 1)[0])


# ---- centres -----------------------------------------------------------------------------------------------------------------------
def test_need_table_equals_its_definition():
    table = th.need_table(200)
    assert table.shape == (3, 201) and table.dtype == np.uint32
    a = np.arange(-15, 16)
    p = np.stack(np.meshgrid(a, a, a, indexing="ij"), axis=-1).reshape(-1, 3)
    norm = (p * p).sum(axis=1)
    for j, delta in enumerate(((1, 0, 0), (1, 1, 0), (1, 1, 1))):
        away = ((p - np.array(delta)) ** 2).sum(axis=1)
        for r in range(1, 201):
            assert table[j, r] == 1 + away[norm < r].max(), (delta, r)
    for delta in ((0, -1, 0), (0, 1, -1), (-1, 1, -1)):                 # the class of an offset is its count of non-zero components
        j = sum(c != 0 for c in delta) - 1
        away = ((p - np.array(delta)) ** 2).sum(axis=1)
        assert all(table[j, r] == 1 + away[norm < r].max() for r in (1, 2, 9, 50, 200))
    assert np.array_equal(th.need_table(50), table[:, :51])              # a shorter request is a prefix of the cached table
    assert th.need_table(10 ** 9).shape == (3, th.NEED_MAX_R + 1)


@pytest.mark.parametrize("name", ["blobs", "blobs_2d", "row", "disc_prism", "debris", "touching", "vessels_crop"])
def test_dropping_centres_changes_nothing(name):
    vol = tc.VOLUMES[name]()
    for value in tc.values_of(vol):
        r = tc.exact_r(vol, value).astype(np.uint32)
        levels = th.table_levels(vol.shape[2], int(r.max()))
        every, kept = th.centres_host(r, None), th.centres_host(r, th.need_table(int(r.max())))
        assert np.array_equal(every, tc.oracle_centres_all(vol, value)) and set(kept.tolist()) <= set(every.tolist())
        maps = [th.resolve_host(th.paint_host(r, c, levels), vol.shape[2])[0].reshape(vol.shape) for c in (every, kept)]
        assert np.array_equal(maps[0], maps[1]) and np.array_equal(maps[0], tc.oracle_cached(name, value))
        if name in ("blobs", "disc_prism", "vessels_crop"):
            assert len(kept) < len(every) // 2                           # and the test does drop: most voxels sit inside a neighbour's ball
        capped = th.centres_host(r, th.need_table(int(r.max()))[:, :3])  # a short table: larger balls are never dropped
        assert set(kept.tolist()) <= set(capped.tolist()) and set(np.flatnonzero(r.reshape(-1) >= 3).tolist()) <= set(capped.tolist())


def test_sparse_table_levels_and_launch_plan():
    assert [th.table_levels(512, r) for r in (1, 2, 5, 1297, 46 * 46 + 1)] == [1, 2, 3, 7, 7] and th.table_levels(40, 10 ** 6) == 6
    assert th.table_levels(4, 100) == 3
    plan = th.launch_plan([100, 50, 2], [10, 300, 1000], (64, 64, 64), launch_rows=19 * 19 * 100)
    assert plan[0] == (0, 100, 100) and plan[1][0] == 100 and plan[1][2] == 50 and plan[-1][1] == 1310
    assert all(a[1] == b[0] for a, b in zip(plan, plan[1:])) and all(e - b >= 64 or e == 1310 for b, e, _ in plan)
    assert th.launch_plan([], [], (4, 4, 4)) == []


# ---- figures -----------------------------------------------------------------------------------------------------------------------
def test_one_thickness_everywhere_has_no_spread():
    """the disc prism reads one thickness at every voxel: from the histogram the standard deviation is exactly 0 (NumPy's, from the
    expanded values, is the rounding error of its mean)"""
    vol = tc.disc_prism()
    t2 = tc.oracle_cached("disc_prism", 1)
    got = th.thickness_scores_from_histogram(th.thickness_histogram(t2, vol, 1, device="cpu"), int(t2.max()), 0.37)
    assert got["std"] == 0.0 and got["min"] == got["max"] == got["mean"] == got["median"] == got["p5"] == got["p95"] == 2.0 * 0.37 * math.sqrt(1297.0)
    assert got["voxels"] == int(vol.sum())


@pytest.mark.parametrize("name,voxel_size", [("blobs", 1.0), ("blobs_2d", 0.37), ("debris", 2.5), ("vessels_crop", 1.0), ("row", 3.0)])
def test_figures_equal_numpy_on_the_expanded_thicknesses(name, voxel_size):
    vol = tc.VOLUMES[name]()
    t2, member = tc.oracle_cached(name, 1 if name != "vessels_crop" else 255), vol != 0
    hist = th.thickness_histogram(t2, vol, int(vol.max()), device="cpu")
    assert hist.sum() == member.sum() and np.array_equal(hist, np.bincount(t2[member].astype(np.int64)))
    got = th.thickness_scores_from_histogram(hist, int(t2.max()), voxel_size)
    want = tc.numpy_figures(t2, member, voxel_size)
    assert got["voxels"] == want["voxels"]
    for key in ("mean", "std", "min", "max", "median", "p5", "p95"):
        assert got[key] == pytest.approx(want[key], rel=1e-12, abs=0.0), key
    assert got["largest_inscribed_diameter"] == 2.0 * voxel_size * math.sqrt(float(tc.exact_r(vol, int(vol.max())).max()))


def test_plates_read_the_stated_bias():
    """distances run between voxel centres: a plate w voxels wide reads w for even w and w + 1 for odd w; a one-voxel line reads 2"""
    for width, reads in zip((1, 2, 3, 4, 5), (2, 2, 4, 4, 6)):
        vol = np.zeros((width + 6, 24, 24), np.uint8)
        vol[3:3 + width] = 1
        t2 = host(vol, 1)
        assert (2.0 * np.sqrt(t2[vol == 1].astype(np.float64)) == reads).all(), width
    line = np.zeros((7, 7, 30), np.uint8)
    line[3, 3, :] = 1
    assert (2.0 * np.sqrt(host(line, 1)[line == 1].astype(np.float64)) == 2).all()


# ---- settings, refusals --------------------------------------------------------------------------------------------------------------
def test_settings_defaults_and_parsing():
    assert th.thickness_settings(SimpleNamespace()) == dict(active=False, values=None, voxel_size=1.0, save_volume=False, max_work=th.DEFAULT_MAX_WORK)
    on = th.thickness_settings(SimpleNamespace(thickness_map=True, thickness_values=[3, 1, 3], thickness_voxel_size=0.5, thickness_save_volume=True,
                                               thickness_max_work=1000))
    assert on == dict(active=True, values=[1, 3], voxel_size=0.5, save_volume=True, max_work=1000)
    assert th.thickness_settings(SimpleNamespace(measure_voxel_size=0.25))["voxel_size"] == 0.25
    assert th.thickness_settings(SimpleNamespace(measure_voxel_size=[2.0, 1.0, 1.0]))["voxel_size"] == 1.0     # not a single number: not taken over
    assert th.thickness_settings(SimpleNamespace(measure_voxel_size=0.25, thickness_voxel_size=[2]))["voxel_size"] == 2.0
    assert th.thickness_settings(SimpleNamespace(thickness_values=7))["values"] == [7]
    with pytest.raises(ValueError, match="isotropic"):
        th.thickness_settings(SimpleNamespace(thickness_voxel_size=[2.0, 1.0, 1.0]))
    for bad in (dict(thickness_voxel_size=0), dict(thickness_voxel_size=-1.0), dict(thickness_values=[1, 256]), dict(thickness_values=[-1]),
                dict(thickness_max_work=0)):
        with pytest.raises(ValueError):
            th.thickness_settings(SimpleNamespace(**bad))
    shipped = (REPO / "volseg-settings" / "2d_model_predict_settings.yaml").read_text()
    for key in ("thickness_map", "thickness_values", "thickness_voxel_size", "thickness_save_volume", "thickness_max_work"):
        assert f"# {key}:" in shipped                                # documented, commented out: the shipped settings measure nothing
    from volume_segmantics_amd.data import get_settings_data
    assert not th.thickness_settings(get_settings_data(REPO / "volseg-settings" / "2d_model_predict_settings.yaml"))["active"]


def test_error_cases():
    vol = tc.blobs()
    with pytest.raises(ValueError, match="uint8"):
        host(vol, 256)
    with pytest.raises(TypeError):
        host(vol.astype(np.float32), 1)
    huge = np.lib.stride_tricks.as_strided(np.zeros(1, np.uint8), shape=(1 << 11, 1 << 10, 1 << 10), strides=(0, 0, 0))
    with pytest.raises(ValueError, match="2\\^31"):
        host(huge, 1)
    with pytest.raises(ValueError, match="2\\^32"):
        host(np.lib.stride_tricks.as_strided(np.zeros(1, np.uint8), shape=(1, 2, 70000), strides=(0, 0, 0)), 1)
    with pytest.raises(ValueError, match="shape"):
        th.thickness_histogram(np.zeros((2, 2), np.uint32), vol, 1, device="cpu")


def test_work_bound_raises_and_names_the_span_count():
    vol = tc.blobs()
    rows = th.thickness_label_volume(vol, SimpleNamespace(), device="cpu")["values"][1]["row_spans"]
    assert rows > 100
    with pytest.raises(ValueError, match=f"paints {rows} row spans, more than thickness_max_work = {rows - 1}"):
        host(vol, 1, max_work=rows - 1)
    assert np.array_equal(host(vol, 1, max_work=rows), tc.oracle_cached("blobs", 1))
    with pytest.raises(ValueError, match="thickness_max_work"):
        th.thickness_label_volume(vol, SimpleNamespace(thickness_max_work=5), device="cpu")


# ---- files, fixture, command, manager ------------------------------------------------------------------------------------------------
def test_written_files(tmp_path):
    vol = tc.touching()
    t = th.thickness_label_volume(vol, SimpleNamespace(thickness_voxel_size=0.5, thickness_save_volume=True), device="cpu")
    assert list(t["values"]) == [1, 2] and t["shape"] == list(vol.shape) and t["volume"].dtype == np.float32
    assert np.array_equal(t["volume"], (2.0 * 0.5 * np.sqrt(t["squared"].astype(np.float64))).astype(np.float32)) and not t["volume"][vol == 0].any()
    written = th.write_thickness(tmp_path / "seg", t)
    assert [p.name for p in written] == ["seg_thickness.csv", "seg_thickness.json"]
    doc = json.loads(written[1].read_text())
    assert doc["settings"] == t["settings"] and doc["shape"] == list(vol.shape) and list(doc["values"]) == ["1", "2"]
    rows = list(csv.reader(written[0].open()))
    assert rows[0] == ["value", "voxels"] + list(th.FIGURES) + ["centres", "row_spans"] and [r[0] for r in rows[1:]] == ["1", "2"]
    for line, value in zip(rows[1:], (1, 2)):
        entry, figures = doc["values"][str(value)], t["values"][value]["figures"]
        squared, count = np.array(entry["histogram"]["squared_thickness"]), np.array(entry["histogram"]["count"])
        assert (count > 0).all() and count.sum() == entry["voxels"] == int((vol == value).sum()) == int(line[1])
        hist = np.zeros(squared.max() + 1, np.int64)
        hist[squared] = count
        assert np.array_equal(hist, np.bincount(tc.oracle_cached("touching", value)[vol == value].astype(np.int64)))
        again = th.thickness_scores_from_histogram(hist, entry["max_squared_radius"], 0.5)      # the file reproduces its own figures to the bit
        for k, name in enumerate(th.FIGURES):
            assert entry[name] == figures[name] == again[name] and float(line[2 + k]) == figures[name]
    assert th.thickness_summary_text(t).count("\n") == 3
    nothing = th.thickness_label_volume(tc.filled(), SimpleNamespace(), device="cpu")
    doc = json.loads(th.write_thickness(tmp_path / "solid", nothing)[1].read_text())
    assert doc["values"]["3"]["mean"] is None and doc["values"]["3"]["voxels"] == 120 and doc["values"]["3"]["histogram"]["count"] == [120]


def test_vessels_crop_against_the_committed_figures():
    """tests/golden/thickness_vessels.json was recorded from the oracle (tests/thickness_cases.py as a program), not from this route"""
    want = tc.vessels_expected()
    assert want["crop"] == tc.CROP
    vol = tc.vessels_crop()
    t = th.thickness_label_volume(vol, SimpleNamespace(), device="cpu")
    assert list(t["values"]) == [255]
    row = t["values"][255]
    used = np.flatnonzero(row["histogram"])
    assert used.tolist() == want["histogram"]["squared_thickness"] and row["histogram"][used].tolist() == want["histogram"]["count"]
    assert row["max_squared_radius"] == want["max_squared_radius"] and row["figures"]["voxels"] == want["figures"]["voxels"]
    for name in th.FIGURES:
        assert row["figures"][name] == pytest.approx(want["figures"][name], rel=1e-12, abs=0.0), name


def test_thickness_command_on_an_hdf5_file(tmp_path):
    """the command measures on a host without a GPU and without thickness_map"""
    from volume_segmantics_amd.scripts import thickness_2d_prediction
    from volume_segmantics_amd.utilities import base_data_utils as utils
    vol = np.array([0, 7, 200], dtype=np.uint8)[tc.touching()]
    (tmp_path / "volseg-settings").mkdir()
    (tmp_path / "volseg-settings" / "2d_model_predict_settings.yaml").write_text("thickness_values: [200]\nthickness_save_volume: true\nmeasure_voxel_size: 0.5\n")
    utils.save_data_to_hdf5(vol, tmp_path / "pred.h5")
    thickness_2d_prediction.main([str(tmp_path / "pred.h5"), "--data_dir", str(tmp_path)])
    assert {p.name for p in tmp_path.iterdir()} == {"volseg-settings", "pred.h5", "pred_thickness.csv", "pred_thickness.json", "pred_thickness.h5"}
    doc = json.loads((tmp_path / "pred_thickness.json").read_text())
    assert doc["settings"]["voxel_size"] == 0.5 and list(doc["values"]) == ["200"]
    saved = utils.get_numpy_from_path(tmp_path / "pred_thickness.h5", internal_path="/data")[0]
    want = tc.oracle_cached("touching", 2)
    assert saved.dtype == np.float32 and np.array_equal(saved, np.sqrt(want.astype(np.float64)).astype(np.float32))
    thickness_2d_prediction.main([str(tmp_path / "pred.h5"), "--data_dir", str(tmp_path), "--output", str(tmp_path / "other")])
    assert (tmp_path / "other_thickness.json").read_bytes() == (tmp_path / "pred_thickness.json").read_bytes()
    for bad in ([str(tmp_path / "missing.h5")], [str(tmp_path / "pred.h5"), "--output", str(tmp_path / "nowhere" / "stem")], []):
        with pytest.raises(SystemExit) as stop:
            thickness_2d_prediction.main(bad)
        assert stop.value.code == 2


def test_manager_keys_absent_and_one_hot(tmp_path, monkeypatch):
    """without the key the manager's thickness step is not entered and every output is as before; with it the files are written;
    one_hot with thickness_map is refused"""
    from volume_segmantics_amd.model.operations import vol_seg_prediction_manager as pm
    assert [step.name for step in pm.LABEL_STEPS] == ["clean", "measure", "mesh", "thickness"]
    labels = tc.touching()
    fake = SimpleNamespace(_predict_single_axis=lambda vol, axis: (labels, None), model_device_num=0)
    settings = SimpleNamespace(one_hot=False, quality="low", prediction_axis="Z", output_probs=False)
    manager = pm.VolSeg2DPredictionManager.__new__(pm.VolSeg2DPredictionManager)
    manager.predictor, manager.settings, manager.data_vol, manager.input_data_chunking = fake, settings, labels, True
    real = th.thickness_label_volume
    monkeypatch.setattr(th, "thickness_label_volume", lambda *a, **k: pytest.fail("measured without the key"))
    (tmp_path / "off").mkdir()
    (tmp_path / "on").mkdir()
    manager.predict_volume_to_path(tmp_path / "off" / "seg.h5")
    settings.thickness_map = False
    manager.predict_volume_to_path(tmp_path / "off" / "seg.h5")
    assert manager.last_thickness is None and [p.name for p in (tmp_path / "off").iterdir()] == ["seg.h5"]
    monkeypatch.setattr(th, "thickness_label_volume", lambda vol, s, device=None: real(vol, s, device="cpu"))
    settings.thickness_map, settings.thickness_save_volume = True, True
    same = manager.predict_volume_to_path(tmp_path / "on" / "seg.h5")
    assert np.array_equal(same, labels)
    assert sorted(p.name for p in (tmp_path / "on").iterdir()) == ["seg.h5", "seg_thickness.csv", "seg_thickness.h5", "seg_thickness.json"]
    assert (tmp_path / "on" / "seg.h5").read_bytes() == (tmp_path / "off" / "seg.h5").read_bytes()
    want = tc.oracle_cached("touching", 1).astype(np.int64) + tc.oracle_cached("touching", 2)
    assert np.array_equal(manager.last_thickness["squared"], want) and list(manager.last_thickness["values"]) == [1, 2]
    settings.one_hot = True
    with pytest.raises(ValueError, match="one_hot.*thickness_map"):
        manager.predict_volume_to_path(None)
