"""The host side of utilities/components.py (no GPU): the settings keys, the host routes - scipy.ndimage.label where scipy imports and
the NumPy propagation, which must agree - against the flood-fill oracle and the per-component cleanup oracle of
tests/components_cases.py, the committed vessels figures, the report files and the clean command as a fresh process."""
import csv
import json
import os
import subprocess
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import components_cases as cc
from volume_segmantics_amd.utilities import components as co

REPO = Path(__file__).resolve().parent.parent
SMALL_SHAPES = [(1, 1, 1), (7, 1, 5), (3, 4, 1), (1, 1, 37), (2, 3, 2), (5, 7, 9), (1, 12, 20)]


def small_volumes():
    for shape in SMALL_SHAPES:
        for k, density, seed in ((2, 0.5, 1), (4, 0.5, 2), (4, 0.05, 3)):
            yield cc.random_labels(shape, k, density, seed)
    yield cc.checkerboard((4, 5, 6))
    yield cc.shells((7, 8, 9))
    yield cc.snake_rows((3, 7, 6))


# ---- settings ----------------------------------------------------------------------------------------------------------------------
def test_settings_defaults_and_parsing():
    assert co.postprocess_settings(SimpleNamespace()) == dict(active=False, min_object_size=0, keep_largest=False, fill_holes=0, connectivity=6)
    off = SimpleNamespace(postprocess_min_object_size=0, postprocess_keep_largest=False, postprocess_fill_holes=0, postprocess_connectivity=26)
    assert not co.postprocess_settings(off)["active"] and co.postprocess_settings(off)["connectivity"] == 26
    assert not co.postprocess_settings(SimpleNamespace(postprocess_min_object_size={1: 0}, postprocess_keep_largest={2: False}))["active"]
    assert not co.postprocess_settings(SimpleNamespace(postprocess_min_object_size=None, postprocess_fill_holes=None))["active"]
    for key, value in (("postprocess_min_object_size", 5), ("postprocess_keep_largest", True), ("postprocess_fill_holes", 3),
                       ("postprocess_min_object_size", {2: 7}), ("postprocess_keep_largest", {1: True})):
        assert co.postprocess_settings(SimpleNamespace(**{key: value}))["active"], key
    with pytest.raises(ValueError, match="6, 18 or 26"):
        co.postprocess_settings(SimpleNamespace(postprocess_connectivity=8))
    shipped = (REPO / "volseg-settings" / "2d_model_predict_settings.yaml").read_text()
    for key in ("postprocess_min_object_size", "postprocess_keep_largest", "postprocess_fill_holes", "postprocess_connectivity"):
        assert f"# {key}:" in shipped                                # documented, commented out: the shipped settings run nothing
    from volume_segmantics_amd.data import get_settings_data
    assert not co.postprocess_settings(get_settings_data(REPO / "volseg-settings" / "2d_model_predict_settings.yaml"))["active"]


def test_per_value_settings():
    vol = cc.cleanup_scene()
    scalar, _ = co.clean_label_volume(vol, min_object_size=28, device="cpu")
    mapped, _ = co.clean_label_volume(vol, min_object_size={c: 28 for c in (1, 2, 3)}, device="cpu")
    assert np.array_equal(scalar, mapped) and not (scalar == 2).any() and not (scalar == 3).any() and (scalar == 1).any()
    only_2, report = co.clean_label_volume(vol, keep_largest={2: True}, device="cpu")
    assert (only_2 == 2).sum() == cc.SCENE["twin"] and only_2[25, 5, 5] == 2 and only_2[25, 5, 40] == 0     # the tie goes to the lower root
    assert report["keep_largest"] == [2] and report["values"]["2"]["components_cleared"] == 2
    assert np.array_equal(only_2 == 1, vol == 1) and np.array_equal(only_2 == 3, vol == 3)
    with pytest.raises(ValueError, match="negative"):
        co.clean_label_volume(vol, min_object_size=-1, device="cpu")
    with pytest.raises(ValueError, match="uint8"):
        co.clean_label_volume(vol, min_object_size={300: 1}, device="cpu")
    with pytest.raises(ValueError, match="connectivity 7"):
        co.label_components(vol, 7, device="cpu")
    with pytest.raises(ValueError, match="do not fit uint8"):
        co.label_components(vol.astype(np.int32) - 1, device="cpu")
    with pytest.raises(TypeError, match="integer"):
        co.label_components(vol.astype(np.float32), device="cpu")
    with pytest.raises(ValueError, match="2\\^31"):
        co.label_components(np.broadcast_to(np.zeros(1, np.uint8), (2048, 1024, 1024)), device="cpu")


# ---- the host routes ---------------------------------------------------------------------------------------------------------------
def test_oracles_agree_with_each_other():
    for vol in small_volumes():
        for c in cc.CONNECTIVITIES:
            got = cc.scipy_roots(vol, c)
            if got is not None:
                assert np.array_equal(got, cc.flood_roots(vol, c)), (vol.shape, c)


def test_host_routes_against_the_flood_fill():
    for vol in small_volumes():
        for c in cc.CONNECTIVITIES:
            want = cc.flood_roots(vol, c)
            got = co.label_components(vol, c, device="cpu")
            assert got.dtype == np.int32 and got.shape == vol.shape and np.array_equal(got, want), (vol.shape, c)
            assert np.array_equal(co._roots_host(vol, c, use_scipy=False), want), (vol.shape, c)      # the NumPy route on its own


def test_scipy_route_and_numpy_route_give_equal_results():
    """the route a host takes by itself (scipy where it imports) against the NumPy route, on volumes beyond the flood fill's reach"""
    for vol in (cc.random_labels((9, 17, 33), 4, 0.5, 7), cc.shells((9, 11, 17)), cc.snake_rows((5, 9, 30))):
        for c in cc.CONNECTIVITIES:
            assert np.array_equal(co._roots_host(vol, c), co._roots_host(vol, c, use_scipy=False)), (vol.shape, c)


def test_lower_dimensional_volumes_and_wide_dtypes():
    plane = cc.random_labels((1, 12, 20), 2, 0.5, 4)[0]
    assert np.array_equal(co.label_components(plane, 18, device="cpu"), cc.flood_roots(plane[None], 18)[0])
    assert np.array_equal(co.label_components(plane.astype(np.int64), 18, device="cpu"), co.label_components(plane, 18, device="cpu"))
    row = plane[3]
    assert np.array_equal(co.label_components(row, device="cpu"), cc.flood_roots(row[None, None], 6)[0, 0])
    assert np.array_equal(co.label_components(plane.astype(bool), device="cpu"), co.label_components(plane, device="cpu"))


def test_component_table():
    vol = cc.cleanup_scene()
    table = co.component_table(vol, 6, device="cpu")
    assert sorted(table) == [0, 1, 2, 3]
    assert table[2] == {"components": 3, "sizes": [27, 27, 4]} and table[3] == {"components": 1, "sizes": [26]}
    assert table[0]["components"] == 5 and table[0]["sizes"][1:] == [5, 4, 3, 1]
    assert sum(sum(t["sizes"]) for t in table.values()) == vol.size


CLEANUPS = [dict(), dict(hole_max=5), dict(hole_max=4), dict(min_size={3: 26}, hole_max=1), dict(min_size={3: 27}, hole_max=1),
            dict(min_size={2: 5}, hole_max=3), dict(keep_largest={2}, hole_max=600), dict(min_size={1: 100, 2: 5, 3: 27}, keep_largest={1, 2}, hole_max=600),
            dict(min_size={0: 10, 2: 28}, hole_max=100, background=1)]


@pytest.mark.parametrize("connectivity", cc.CONNECTIVITIES)
def test_cleanup_against_the_oracle(connectivity):
    vol = cc.cleanup_scene()
    for case in CLEANUPS:
        got, report = co.clean_label_volume(vol, case.get("min_size", 0), {c: True for c in case.get("keep_largest", ())}, case.get("hole_max", 0),
                                            connectivity, case.get("background", 0), device="cpu")
        want, totals, rows = cc.oracle_clean(vol, connectivity, case.get("min_size"), case.get("keep_largest"), case.get("hole_max", 0),
                                             case.get("background", 0))
        assert got.dtype == np.uint8 and np.array_equal(got, want), case
        assert report["values"] == rows and [report["holes_filled"], report["voxels_filled"]] == totals[2:], case
        assert sum(r["components_cleared"] for r in rows.values()) == totals[0] and sum(r["voxels_cleared"] for r in rows.values()) == totals[1]


def test_cleanup_rules_one_by_one():
    vol = cc.cleanup_scene()
    got, report = co.clean_label_volume(vol, fill_holes=600, device="cpu")
    assert (got[8, 8, 10:15] == 1).all() and (got[12, 12, 24:27] == 2).all() and got[33, 11, 11] == 3      # each takes the value in front of its root
    assert (got[32:34, 2:4, 71] == 0).all()                         # open to the boundary: never filled
    assert report["holes_filled"] == 3 and report["voxels_filled"] == 9
    got, report = co.clean_label_volume(vol, min_object_size={3: 27}, fill_holes=600, device="cpu")
    assert (got[32:35, 10:13, 10:13] == 0).all() and report["holes_filled"] == 2      # the hole of a cleared object stays background
    assert co.clean_label_volume(vol, fill_holes=4, device="cpu")[1]["holes_filled"] == 2             # hole A (5 voxels) is one too large
    assert (co.clean_label_volume(vol, min_object_size={3: 26}, device="cpu")[0] == 3).sum() == 26    # at the size: kept
    same, report = co.clean_label_volume(vol, device="cpu")
    assert np.array_equal(same, vol) and report["holes_filled"] == 0 and all(r["components_cleared"] == 0 for r in report["values"].values())
    lone = np.zeros((1, 1, 1), np.uint8)
    assert co.clean_label_volume(lone, fill_holes=5, device="cpu")[0].tolist() == [[[0]]]               # voxel 0 has no voxel in front of it


def test_vessels_fixture_against_the_committed_figures():
    vol = cc.vessels()
    expected = cc.vessels_expected()["connectivity"]
    head = {6: ([5099604, 374998, 90300, 87335, 74900], 15, [10896118, 543, 290, 106, 99], 28),
            18: ([5099604, 374998, 90300, 87335, 74900], 15, [10896133, 543, 389, 106, 94], 18),
            26: ([5474602, 90300, 87335, 74900, 32479], 14, [10896134, 543, 389, 106, 94], 16)}
    for c, (fg, nfg, bg, nbg) in head.items():
        table = expected[str(c)]["table"]
        assert table["255"]["components"] == nfg and table["255"]["sizes"][:5] == fg and table["0"]["components"] == nbg and table["0"]["sizes"][:5] == bg
    got = co.component_table(vol, 26, device="cpu")                 # one connectivity here; the GPU test does all three
    assert {str(k): v for k, v in got.items()} == expected["26"]["table"]
    out, report = co.clean_label_volume(vol, fill_holes=600, connectivity=26, device="cpu")
    want = expected["26"]["cleanups"]["fill_holes_600"]
    assert [report["holes_filled"], report["voxels_filled"]] == [want["holes_filled"], want["voxels_filled"]] and report["values"] == want["values"]
    assert {str(int(k)): int(n) for k, n in zip(*np.unique(out, return_counts=True))} == want["voxels_of_value"]


# ---- report files and the command --------------------------------------------------------------------------------------------------
def test_report_files(tmp_path):
    vol = cc.cleanup_scene()
    _, report = co.clean_label_volume(vol, min_object_size={3: 27}, keep_largest={2: True}, fill_holes=10, connectivity=18, device="cpu")
    written = co.write_component_report(tmp_path / "seg", report)
    assert [p.name for p in written] == ["seg_components.json", "seg_components.csv"]
    assert json.loads(written[0].read_text()) == report
    assert report["connectivity"] == 18 and report["fill_holes"] == 10 and report["min_object_size"] == {"3": 27} and report["keep_largest"] == [2]
    rows = list(csv.reader(written[1].read_text().splitlines()))
    assert rows[0] == ["label_value", "components", "voxels", "components_cleared", "voxels_cleared", "components_kept", "voxels_kept"]
    assert [r[0] for r in rows[1:]] == ["0", "1", "2", "3", "holes"]
    assert rows[3][1:] == ["3", "58", "2", "31", "1", "27"] and rows[5][1:3] == [str(report["holes_filled"]), str(report["voxels_filled"])]
    assert "holes filled" in co.component_report_table(report)


def test_clean_command_as_a_fresh_process(tmp_path):
    from volume_segmantics_amd.utilities import base_data_utils as utils
    vol = cc.cleanup_scene()
    raw = np.array([0, 7, 100, 200], dtype=np.uint8)[vol]           # label VALUES, as a prediction file holds them
    (tmp_path / "volseg-settings").mkdir()
    (tmp_path / "volseg-settings" / "2d_model_predict_settings.yaml").write_text(
        "postprocess_min_object_size: {200: 27}\npostprocess_keep_largest: {100: true}\npostprocess_fill_holes: 10\npostprocess_connectivity: 18\n")
    utils.save_data_to_hdf5(raw, tmp_path / "pred.h5")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([str(REPO)] + [p for p in [os.environ.get("PYTHONPATH")] if p]))
    cmd = [sys.executable, "-m", "volume_segmantics_amd.scripts.clean_2d_prediction"]
    done = subprocess.run(cmd + [str(tmp_path / "pred.h5"), "--data_dir", str(tmp_path)], cwd=REPO, env=env, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-2000:]
    assert {p.name for p in tmp_path.iterdir()} == {"volseg-settings", "pred.h5", "pred_cleaned.h5", "pred_components.json", "pred_components.csv"}
    cleaned = utils.numpy_from_hdf5(tmp_path / "pred_cleaned.h5")[0]
    want, totals, rows = cc.oracle_clean(raw, 18, {200: 27}, {100}, 10)
    assert cleaned.dtype == np.uint8 and np.array_equal(cleaned, want)
    report = json.loads((tmp_path / "pred_components.json").read_text())
    assert report["values"] == rows and [report["holes_filled"], report["voxels_filled"]] == totals[2:] and report["connectivity"] == 18

    from volume_segmantics_amd.scripts import clean_2d_prediction
    from volume_segmantics_amd.utilities import arg_parsing
    clean_2d_prediction.main([str(tmp_path / "pred.h5"), "--data_dir", str(tmp_path), "--output", str(tmp_path / "other.npy")])
    assert np.array_equal(np.load(tmp_path / "other.npy"), want)
    for bad in ([str(tmp_path / "missing.h5")], [str(tmp_path / "pred.h5"), "--output", str(tmp_path / "out.txt")], []):
        with pytest.raises(SystemExit) as stop:
            arg_parsing.parse_cleaning_args(bad)
        assert stop.value.code == 2
