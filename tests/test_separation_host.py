"""The host side of utilities/separation.py (no GPU): parents, basins, the pair table and the objects of the host route integer for
integer against the brute-force oracle of tests/separation_cases.py on every named scene, the two ends of the depth, the committed
vessels figures, the surface identity between objects and components, the settings keys, the refusals, the files of the command and
the manager with and without the key.  Nothing here has a tolerance."""
import csv
import json
from types import SimpleNamespace

import numpy as np
import pytest

import components_cases as cc
import measurement_cases as mc
import separation_cases as sc
import thickness_cases as tc
from volume_segmantics_amd.utilities import measurements as me
from volume_segmantics_amd.utilities import separation as sp
from volume_segmantics_amd.utilities import surface_distance as sd

INF = float("inf")


def host(vol, **kw):
    return sp.separate_objects(vol, device="cpu", **kw)


def contacts_as_dict(c):
    return {(int(a), int(b)): [int(v), int(n)] + [int(x) for x in f]
            for a, b, v, n, f in zip(c["root_a"], c["root_b"], c["value"], c["neck_squared"], c["faces"])}


# ---- the stages and the objects ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(sc.SCENES))
def test_stages_against_the_oracle(name):
    vol = sc.scene(name)
    for connectivity in cc.CONNECTIVITIES:
        for value in sc.values_of(vol):
            st = sc.stages_cached(name, value, connectivity)
            if st is None:
                continue
            member = vol == value
            r = np.where(member, sd.squared_distance_transform(~member, device="cpu").reshape(vol.shape), 0).astype(np.uint32)
            assert np.array_equal(r, st["r"]), (name, value)
            parent = sp.ascent_parents(r, connectivity)
            assert parent.dtype == np.int32 and np.array_equal(parent.reshape(-1), st["parent"]), (name, value, connectivity)
            basin = sp.basins(parent)
            assert np.array_equal(basin.reshape(-1), st["basin"]), (name, value, connectivity)
            table = sp.basin_pairs(r, basin, connectivity)
            a, b, saddle, faces = sc.rows_as_arrays(st["rows"])
            assert table["count"] == st["count"] and np.array_equal(table["a"], a) and np.array_equal(table["b"], b), (name, value, connectivity)
            assert np.array_equal(table["saddle"], saddle) and np.array_equal(table["faces"], faces), (name, value, connectivity)
            peaks = np.array(sorted(st["peak_r"]), dtype=np.int64)
            for depth in (0.0, 0.5, 1.0, INF):
                rep, merges = sp.merge_basins(peaks, [st["peak_r"][int(p)] for p in peaks], a, b, saddle, depth)
                want, want_merges = sc.oracle_merge(st["rows"], st["peak_r"], depth)
                assert merges == want_merges and rep.tolist() == [want[int(p)] for p in peaks], (name, value, connectivity, depth)


@pytest.mark.parametrize("name", sorted(sc.SCENES))
def test_objects_reports_and_contacts_against_the_oracle(name):
    vol = sc.scene(name)
    for connectivity in cc.CONNECTIVITIES:
        components = cc.oracle_roots(vol, connectivity).reshape(vol.shape)
        for depth in (0.0, 1.0, 2.0, INF):
            got = host(vol, connectivity=connectivity, depth=depth)
            objects, report, contacts = sc.separate_cached(name, connectivity, depth)
            assert got["objects"].dtype == np.int32 and got["objects"].shape == vol.shape
            assert np.array_equal(got["objects"].reshape(-1), objects), (name, connectivity, depth)
            assert contacts_as_dict(got["contacts"]) == contacts, (name, connectivity, depth)
            for value, want in report.items():
                have = got["report"][str(value)]
                assert have["components"] == want["components"] and have["separated"] == want["separated"]
                if want["separated"]:
                    assert {k: have[k] for k in ("basins", "pair_rows", "merges", "objects")} == {k: want[k] for k in ("basins", "pair_rows", "merges", "objects")}
                    assert have["why"] is None
                else:
                    assert "no other value" in have["why"] and have["objects"] == have["components"]
            # a refinement of the components: every object lies in one component, and its id is its lowest voxel
            flat = got["objects"].reshape(-1)
            assert np.array_equal(components.reshape(-1)[flat], components.reshape(-1)) and (flat <= np.arange(flat.size)).all()
            assert np.array_equal(flat[flat], flat)
            if depth == INF:
                assert np.array_equal(got["objects"], components) and len(got["contacts"]["root_a"]) == 0
        raw = host(vol, connectivity=connectivity, depth=0.0)["objects"].reshape(-1)
        for value in sc.values_of(vol):
            st = sc.stages_cached(name, value, connectivity)
            if st is not None:                                        # depth 0: the raw basins, named by their lowest voxel
                inside = st["basin"] >= 0
                lowest = {}
                for v in np.flatnonzero(inside).tolist():
                    lowest.setdefault(int(st["basin"][v]), v)
                assert np.array_equal(raw[inside], [lowest[int(b)] for b in st["basin"][inside]])


def test_what_the_scenes_are_for():
    assert [sc.separate_cached("two_balls", 26, d)[1][1]["objects"] for d in (0.0, 1.0, 2.0)] == [2, 2, 2]
    assert cc.oracle_roots(sc.scene("two_balls"), 26).max() == cc.oracle_roots(sc.scene("two_balls"), 26)[sc.scene("two_balls") == 1].min()      # one component
    cylinder = [sc.separate_cached("cylinder", 26, d)[1][1] for d in (0.0, 1.0, 2.0)]
    assert cylinder[0]["objects"] > 1 and cylinder[1]["objects"] == 1 and cylinder[2]["objects"] == 1      # the ridge's ripple stays below one voxel
    slab = sc.stages_cached("slab_z", 1, 26)
    on_plateau = np.flatnonzero(slab["r"].reshape(-1) == slab["r"].max())
    assert len(set(slab["basin"][on_plateau].tolist())) == 1 and len(on_plateau) > 128      # one peak takes the whole mid-plane: long chains
    assert len(sc.stages_cached("ties", 1, 6)["peak_r"]) > 1 and sc.separate_cached("ties", 6, 0.5)[1][1]["objects"] == 1      # plateau peaks join at any depth
    face = sc.stages_cached("peak_on_face", 1, 26)
    assert all(p < 15 * 15 for p in face["peak_r"])                  # the peak lies in the plane z = 0
    debris = sc.stages_cached("debris_rows", 1, 6)
    basin = debris["basin"].reshape(sc.scene("debris_rows").shape)[:, :, :64]      # the first 64 voxels of every row: one wave's lanes
    along_x = (basin[:, :, 1:] >= 0) & (basin[:, :, :-1] >= 0) & (basin[:, :, 1:] != basin[:, :, :-1])
    assert max(len(set(row[row >= 0].tolist())) for row in basin.reshape(-1, 64)) > 8      # beyond the ballot rounds of the relabelling
    assert along_x.reshape(-1, 63).sum(axis=1).max() > 8             # and of the pair table: those insert on their own
    report = sc.separate_cached("two_values", 6, 1.0)[1]
    assert report[1]["objects"] == 2 and report[2]["objects"] == 2
    got = host(sc.scene("two_values"), connectivity=6, values=[2])    # one value only: the other keeps its component
    assert got["report"].keys() == {"2"}
    assert len(np.unique(got["objects"][sc.scene("two_values") == 1])) == 1 and len(np.unique(got["objects"][sc.scene("two_values") == 2])) == 2


def test_absent_values_full_volumes_and_arguments():
    vol = sc.scene("two_balls")
    got = host(vol, values=[1, sc.ABSENT])
    assert got["report"][str(sc.ABSENT)] == dict(components=0, separated=False, why="the volume does not hold the value", basins=0, pair_rows=0,
                                                 adjacent_pairs=0, merges=0, objects=0)
    filled = host(sc.scene("filled"))
    assert filled["report"]["3"]["separated"] is False and filled["report"]["3"]["components"] == 1 and not filled["objects"].any()
    assert host(np.zeros((3, 4, 5), np.uint8))["report"] == {}
    assert host(vol, values=0)["report"]["0"]["separated"]            # the background is separated only when it is named
    plane = host(sc.scene("plane")[0])                                # a 2-D volume keeps its shape
    assert plane["objects"].shape == (30, 34)
    for bad in (dict(depth=-1.0), dict(depth=float("nan")), dict(values=[256]), dict(connectivity=7)):
        with pytest.raises(ValueError):
            host(vol, **bad)
    assert sp.table_slots(0, 1) == 2 and sp.table_slots(100, 3) == 8 and sp.table_slots(5, 100) == 16 and sp.table_slots(1 << 20, 1 << 20) == 1 << 21


def test_too_many_pairs_are_refused():
    vol = cc.random_labels((8, 16, 32), 4, 1.0, 7)                    # debris
    rows = host(vol, values=[1], max_pairs=None)["report"]["1"]["pair_rows"]
    assert rows > 100
    with pytest.raises(ValueError, match=f"value 1 has {rows} rows, more than measure_separate_max_pairs = 100"):
        host(vol, values=[1], max_pairs=100)
    assert host(vol, values=[1], max_pairs=rows)["report"]["1"]["pair_rows"] == rows


# ---- the committed figures -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", cc.CONNECTIVITIES)
def test_vessels_crop_against_the_committed_figures(connectivity):
    doc = sc.vessels_expected()
    assert doc["crop"] == tc.CROP and doc["value"] == 255
    vol = tc.vessels_crop()
    assert int((vol == 255).sum()) == doc["voxels"]
    expected = doc["connectivity"][str(connectivity)]
    for depth in sc.DEPTHS:
        got = host(vol, values=[255], connectivity=connectivity, depth=depth)
        report, want = got["report"]["255"], expected["objects"][str(depth)]
        assert (report["basins"], report["pair_rows"], report["adjacent_pairs"]) == (expected["basins"], expected["pair_rows"], expected["adjacent_pairs"])
        assert (report["objects"], report["merges"], len(got["contacts"]["root_a"])) == (want["count"], want["merges"], want["contacts"])
        roots, sizes = np.unique(got["objects"][vol == 255], return_counts=True)
        assert roots.tolist() == want["roots"] and sizes.tolist() == want["voxels"]


# ---- measuring the objects -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["two_balls", "three_balls", "rows_65", "two_values", "random", "plane"])
def test_measured_objects_and_the_surface_identity(name):
    vol = np.asarray(sc.scene(name))
    for connectivity, depth in ((6, 0.0), (26, 1.0)):
        separate = dict(values=None, depth=depth, max_pairs=None)
        raw = me.measure_components(vol, connectivity=connectivity, device="cpu", separate=separate)
        objects, _, contacts = sc.separate_cached(name, connectivity, depth)
        roots = np.flatnonzero(objects == np.arange(objects.size))
        roots = roots[vol.reshape(-1)[roots] != 0]
        order = np.lexsort((roots, vol.reshape(-1)[roots]))
        assert raw["roots"].tolist() == roots[order].tolist() and raw["values"].tolist() == vol.reshape(-1)[roots[order]].tolist()
        row_of_root = np.full(objects.size, -1, dtype=np.int32)
        row_of_root[raw["roots"]] = np.arange(len(raw["roots"]))
        want = mc.oracle_rows(vol, objects.reshape(vol.shape), row_of_root, len(roots))      # everything but the faces: those it takes from the values
        assert np.array_equal(raw["table"][:, :16], want[:, :16]) and np.array_equal(raw["table"][:, 19], want[:, 19])
        plain = me.measure_components(vol, connectivity=connectivity, device="cpu")
        between = np.array([c[2:5] for c in contacts.values()], dtype=np.int64).reshape(-1, 3).sum(axis=0)
        # every contact face is a face of both objects that the components did not count
        assert (raw["table"][:, 16:19].sum(axis=0) == plain["table"][:, 16:19].sum(axis=0) + 2 * between).all(), (name, connectivity, depth)
        assert raw["table"][:, 0].sum() == plain["table"][:, 0].sum()
        ids = me.object_ids(vol, connectivity=connectivity, device="cpu", separate=separate)
        assert np.array_equal(np.bincount(ids.reshape(-1))[1:], raw["table"][:, 0]) and np.array_equal(ids.reshape(-1)[raw["roots"]], np.arange(1, len(roots) + 1))
        same = me.measure_components(vol, connectivity=connectivity, device="cpu", separate=dict(values=None, depth=INF, max_pairs=None))
        mc.assert_raw_equal(same, plain, (name, "depth inf"))          # the id-based faces of a component labelling are the value-based ones
    few = me.measure_components(vol, min_voxels=30, device="cpu", separate=dict(values=None, depth=0.0, max_pairs=None))
    every = me.measure_components(vol, device="cpu", separate=dict(values=None, depth=0.0, max_pairs=None))
    small = every["table"][:, 0] < 30
    assert few["table"][:, 0].tolist() == every["table"][~small, 0].tolist()
    assert few["not_listed_objects"].sum() - every["not_listed_objects"].sum() == small.sum()
    assert few["not_listed_voxels"].sum() - every["not_listed_voxels"].sum() == every["table"][small, 0].sum()


# ---- settings, writers, command, manager -----------------------------------------------------------------------------------------
def test_settings_defaults_and_refusals():
    from volume_segmantics_amd.data import get_settings_data
    assert sp.separation_settings(SimpleNamespace()) == dict(active=False, values=None, depth=1.0, max_pairs=5000000)
    on = sp.separation_settings(SimpleNamespace(measure_separate=True, measure_separate_values=[3, 1], measure_separate_depth=2, measure_separate_max_pairs=10))
    assert on == dict(active=True, values=[1, 3], depth=2.0, max_pairs=10)
    assert sp.separation_settings(SimpleNamespace(measure_separate_values=7))["values"] == [7]
    assert sp.separation_settings(SimpleNamespace(measure_separate_depth="inf"))["depth"] == INF
    assert sp.separation_settings(SimpleNamespace(measure_separate_depth=0))["depth"] == 0.0
    for bad in (dict(measure_separate_depth=-0.5), dict(measure_separate_values=[300]), dict(measure_separate_max_pairs=0)):
        with pytest.raises(ValueError):
            sp.separation_settings(SimpleNamespace(**bad))
    shipped = (mc.cc.GOLDEN.parent.parent / "volseg-settings" / "2d_model_predict_settings.yaml")
    for key in ("measure_separate", "measure_separate_values", "measure_separate_depth", "measure_separate_max_pairs"):
        assert f"# {key}:" in shipped.read_text()                     # documented, commented out
    assert not sp.separation_settings(get_settings_data(shipped))["active"]
    assert me.measurement_settings(SimpleNamespace(measure_separate=True)) == me.measurement_settings(SimpleNamespace())      # its keys stay its own


def test_measure_label_volume_and_the_writers(tmp_path):
    vol = np.asarray(sc.scene("two_values"))
    plain = me.measure_label_volume(vol, SimpleNamespace(measure_separate=False, measure_save_ids=True), device="cpu")
    assert "separation" not in plain and plain["table"]["objects"]["id"].tolist() == [1, 2]
    settings = SimpleNamespace(measure_separate=True, measure_separate_depth=1.0, measure_voxel_size=[2.0, 1.0, 0.5], measure_save_ids=True)
    m = me.measure_label_volume(vol, settings, device="cpu")
    assert m["table"]["objects"]["id"].tolist() == [1, 2, 3, 4] and m["table"]["objects"]["value"].tolist() == [1, 1, 2, 2]
    assert np.array_equal(np.unique(m["ids"]), np.arange(5)) and m["separation"]["settings"] == sp.separation_settings(settings)
    c = m["separation"]["contacts"]
    assert tuple(c) == sp.CONTACT_COLUMNS and c["id_a"].tolist() == [1, 3] and c["id_b"].tolist() == [2, 4] and c["value"].tolist() == [1, 2]
    objects, _, contacts = sc.separate_cached("two_values", 6, 1.0)
    want = [contacts[key] for key in sorted(contacts, key=lambda k: (contacts[k][0], k))]
    assert [c["neck_squared"].tolist(), c["faces_z"].tolist(), c["faces_y"].tolist(), c["faces_x"].tolist()] == [[w[i] for w in want] for i in (1, 2, 3, 4)]
    assert c["contact_area"].tolist() == [w[2] * 0.5 + w[3] * 1.0 + w[4] * 2.0 for w in want]
    assert c["neck_radius"].tolist() == [float(np.sqrt(np.float64(w[1]))) for w in want]
    coordination = np.bincount(np.concatenate([c["id_a"], c["id_b"]]), minlength=5)
    assert coordination.tolist() == [0, 1, 1, 1, 1]                   # the number of rows that name an object
    hidden = me.measure_label_volume(vol, SimpleNamespace(measure_separate=True, measure_min_voxels=10 ** 6), device="cpu")["separation"]["contacts"]
    assert hidden["id_a"].tolist() == [0, 0] and hidden["id_b"].tolist() == [0, 0]      # objects the table does not list
    assert "taken apart at depth 1.0 (2 contacts)" in me.separation_text(m) and me.separation_text(plain) == ""

    written = me.write_measurements(tmp_path / "seg", m["raw"], m["table"], m["settings"], m["separation"])
    assert [p.name for p in written] == ["seg_objects.csv", "seg_objects.json", "seg_object_contacts.csv", "seg_object_contacts.json"]
    doc = json.loads(written[1].read_text())
    assert doc["separation"] == {"settings": dict(active=True, values=None, depth=1.0, max_pairs=5000000), "report": m["separation"]["report"]}
    mc.assert_raw_equal(me.raw_from_json(doc), m["raw"])
    with open(written[2], newline="") as f:
        rows = list(csv.reader(f))
    assert tuple(rows[0]) == sp.CONTACT_COLUMNS and len(rows) == 3 and [int(rows[1][0]), int(rows[1][1]), int(rows[1][2])] == [1, 2, 1]
    assert float(rows[1][6]) == c["contact_area"][0] and float(rows[1][8]) == c["neck_radius"][0]
    again = json.loads(written[3].read_text())
    assert again["columns"] == list(sp.CONTACT_COLUMNS) and len(again["contacts"]) == 2 and again["report"] == m["separation"]["report"]
    before = me.write_measurements(tmp_path / "plain", plain["raw"], plain["table"], plain["settings"])
    assert [p.name for p in before] == ["plain_objects.csv", "plain_objects.json"] and "separation" not in json.loads(before[1].read_text())


def test_measure_command_writes_the_contacts(tmp_path):
    from volume_segmantics_amd.scripts import measure_2d_prediction
    from volume_segmantics_amd.utilities import base_data_utils as utils
    vol = np.asarray(sc.scene("three_balls"))
    (tmp_path / "volseg-settings").mkdir()
    settings = tmp_path / "volseg-settings" / "2d_model_predict_settings.yaml"
    settings.write_text("measure_save_ids: true\nmeasure_connectivity: 26\n")
    utils.save_data_to_hdf5(vol, tmp_path / "pred.h5")
    measure_2d_prediction.main([str(tmp_path / "pred.h5"), "--data_dir", str(tmp_path), "--output", str(tmp_path / "before")])
    assert {p.name for p in tmp_path.iterdir()} == {"volseg-settings", "pred.h5", "before_objects.csv", "before_objects.json", "before_object_ids.h5"}
    settings.write_text("measure_save_ids: true\nmeasure_connectivity: 26\nmeasure_separate: true\nmeasure_separate_values: [1]\nmeasure_separate_depth: 1.0\n")
    measure_2d_prediction.main([str(tmp_path / "pred.h5"), "--data_dir", str(tmp_path)])
    assert {p.name for p in tmp_path.iterdir()} == {"volseg-settings", "pred.h5", "before_objects.csv", "before_objects.json", "before_object_ids.h5",
                                                    "pred_objects.csv", "pred_objects.json", "pred_object_ids.h5", "pred_object_contacts.csv",
                                                    "pred_object_contacts.json"}
    objects, report, contacts = sc.separate_cached("three_balls", 26, 1.0)
    doc = json.loads((tmp_path / "pred_objects.json").read_text())
    assert len(doc["objects"]) == report[1]["objects"] == 3 and len(json.loads((tmp_path / "before_objects.json").read_text())["objects"]) == 1
    assert [o["root"] for o in doc["objects"]] == sorted(set(objects[vol.reshape(-1) == 1].tolist()))
    ids = utils.numpy_from_hdf5(tmp_path / "pred_object_ids.h5")[0]
    assert np.array_equal(ids, me.object_ids(vol, connectivity=26, device="cpu", separate=dict(values=[1], depth=1.0, max_pairs=None)))
    assert len(json.loads((tmp_path / "pred_object_contacts.json").read_text())["contacts"]) == len(contacts)
    settings.write_text("measure_separate: true\nmeasure_separate_max_pairs: 1\n")
    with pytest.raises(ValueError, match="measure_separate_max_pairs = 1"):
        measure_2d_prediction.main([str(tmp_path / "pred.h5"), "--data_dir", str(tmp_path)])


def test_manager_with_and_without_the_key(tmp_path, monkeypatch):
    from volume_segmantics_amd.model.operations import vol_seg_prediction_manager as pm
    from volume_segmantics_amd.utilities import base_data_utils as utils
    assert [step.name for step in pm.LABEL_STEPS] == ["clean", "measure", "mesh", "thickness"]      # separation lives inside the measure step
    labels = np.asarray(sc.scene("two_values"))
    fake = SimpleNamespace(_predict_single_axis=lambda vol, axis: (labels, None), model_device_num=0)
    settings = SimpleNamespace(one_hot=False, quality="low", prediction_axis="Z", output_probs=False, measure_objects=True, measure_save_ids=True)
    manager = pm.VolSeg2DPredictionManager.__new__(pm.VolSeg2DPredictionManager)
    manager.predictor, manager.settings, manager.data_vol, manager.input_data_chunking = fake, settings, labels, True
    run = pm.LABEL_STEPS[1].run
    monkeypatch.setattr(pm, "LABEL_STEPS", tuple(step._replace(run=lambda v, s, device: run(v, s, "cpu")) if step.name == "measure" else step
                                                 for step in pm.LABEL_STEPS))
    for name in ("absent", "off", "on"):
        (tmp_path / name).mkdir()
    with monkeypatch.context() as patch:
        patch.setattr(sp, "separate_prepared", lambda *a, **k: pytest.fail("separated without the key"))
        manager.predict_volume_to_path(tmp_path / "absent" / "seg.h5")
        settings.measure_separate = False
        manager.predict_volume_to_path(tmp_path / "off" / "seg.h5")
    names = ["seg.h5", "seg_object_ids.h5", "seg_objects.csv", "seg_objects.json"]
    assert sorted(p.name for p in (tmp_path / "absent").iterdir()) == names and "separation" not in manager.last_measurements
    for name in names[1:]:
        assert (tmp_path / "off" / name).read_bytes() == (tmp_path / "absent" / name).read_bytes()
    settings.measure_separate = True
    out = manager.predict_volume_to_path(tmp_path / "on" / "seg.h5")
    assert np.array_equal(out, labels)
    assert sorted(p.name for p in (tmp_path / "on").iterdir()) == ["seg.h5", "seg_object_contacts.csv", "seg_object_contacts.json"] + names[1:]
    assert manager.last_measurements["separation"]["report"]["1"]["objects"] == 2
    assert len(json.loads((tmp_path / "on" / "seg_objects.json").read_text())["objects"]) == 4
    assert len(json.loads((tmp_path / "absent" / "seg_objects.json").read_text())["objects"]) == 2
    assert np.array_equal(utils.numpy_from_hdf5(tmp_path / "on" / "seg_object_ids.h5")[0], manager.last_measurements["ids"])
