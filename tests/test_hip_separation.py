"""-m gpu: the stages of csrc/separate.hip through the C ABI, integer for integer against the brute-force oracle of
tests/separation_cases.py on every named scene and under 6, 18 and 26 - parents, basins, the pair count, the pair table (sorted by
key) and the relabelling - then a table that is too small, two runs for the same bits, vs_object_moments against
vs_component_moments and against the host table, the Python route on the device against the host route and the committed vessels
figures, and the manager and the measure command with the keys set.  Every buffer a kernel writes starts out full of garbage and has
one guard element behind it; nothing here has a tolerance."""
import json
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import components_cases as cc
import measurement_cases as mc
import separation_cases as sc
import thickness_cases as tc
from hip_helpers import DEV, lib
from volume_segmantics_amd.utilities import measurements as me
from volume_segmantics_amd.utilities import separation as sp

pytestmark = pytest.mark.gpu

GARBAGE32, GARBAGE64 = -0x01234567, -0x0123456789ABCDEF


def guarded(n, dtype):
    """n elements of garbage and a guard behind them"""
    return torch.full((n + 1,), GARBAGE64 if dtype == torch.int64 else GARBAGE32, dtype=dtype, device=DEV)


def intact(buffer):
    assert int(buffer[-1]) == (GARBAGE64 if buffer.dtype == torch.int64 else GARBAGE32), "the guard element was written"
    return buffer[:-1]


def dev32(a):
    """a host array of 32-bit integers (uint32 bits included) as int32 device memory"""
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).astype(np.int64).astype(np.uint32).view(np.int32)).to(DEV)


def run_parents(r, connectivity):
    L = lib()
    out, r_dev = guarded(r.size, torch.int32), dev32(r)             # inputs stay referenced until the call has run
    L.check(L.lib.vs_separate_parents(L.ptr(r_dev), *r.shape, connectivity, L.ptr(out), L.stream_ptr()))
    return intact(out).cpu().numpy()


def run_basins(parent, shape):
    L = lib()
    buf = guarded(parent.size, torch.int32)
    buf[:-1] = dev32(parent)
    L.check(L.lib.vs_separate_basins(L.ptr(buf), *shape, L.stream_ptr()))
    return intact(buf).cpu().numpy()


def run_pair_count(basin, shape, connectivity):
    L = lib()
    count, basin_dev = guarded(1, torch.int64), dev32(basin)
    L.check(L.lib.vs_separate_pair_count(L.ptr(basin_dev), *shape, connectivity, L.ptr(count), L.stream_ptr()))
    return int(intact(count)[0])


def run_pairs(r, basin, connectivity, slots):
    """(rc, the occupied slots sorted by key as (a, b, saddle, faces), used)"""
    L = lib()
    keys, saddle, faces, used = guarded(slots, torch.int64), guarded(slots, torch.int32), guarded(3 * slots, torch.int32), guarded(2, torch.int64)
    r_dev, basin_dev = dev32(r), dev32(basin)
    rc = L.lib.vs_separate_pairs(L.ptr(r_dev), L.ptr(basin_dev), *r.shape, connectivity, L.ptr(keys), L.ptr(saddle), L.ptr(faces), slots,
                                 L.ptr(used), L.stream_ptr())
    torch.cuda.synchronize()
    keys, saddle, faces, used = (intact(t).cpu().numpy() for t in (keys, saddle, faces, used))
    taken = np.flatnonzero(keys != -1)
    order = taken[np.argsort(keys[taken], kind="stable")]
    k = keys[order].astype(np.int64)
    return rc, (k >> 32, k & 0xFFFFFFFF, saddle[order].astype(np.int64) & 0xFFFFFFFF, faces.reshape(-1, 3)[order].astype(np.int64)), used


def run_relabel(basin, set_of_peak, shape, objects):
    L = lib()
    out = guarded(basin.size, torch.int32)
    out[:-1] = dev32(objects)
    need = int(L.lib.vs_separate_workspace_bytes(*shape))
    assert need == 4 * basin.size
    work = guarded(need // 4, torch.int32)
    basin_dev, set_dev = dev32(basin), dev32(set_of_peak)
    L.check(L.lib.vs_separate_relabel(L.ptr(basin_dev), L.ptr(set_dev), *shape, L.ptr(out), L.ptr(work), need, L.stream_ptr()))
    intact(work)
    return intact(out).cpu().numpy()


# ---- the stages through the C ABI ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(sc.SCENES))
def test_stages_against_the_oracle(name):
    vol = sc.scene(name)
    for connectivity in cc.CONNECTIVITIES:
        for value in sc.values_of(vol):
            st = sc.stages_cached(name, value, connectivity)
            if st is None:                                            # the value fills the volume: there is no distance map to climb
                continue
            what = (name, value, connectivity)
            parent = run_parents(st["r"], connectivity)
            assert np.array_equal(parent, st["parent"]), (what, np.flatnonzero(parent != st["parent"])[:8])
            basin = run_basins(st["parent"], vol.shape)
            assert np.array_equal(basin, st["basin"]), (what, np.flatnonzero(basin != st["basin"])[:8])
            assert run_pair_count(st["basin"], vol.shape, connectivity) == st["count"], what
            slots = sp.table_slots(st["count"], len(st["peak_r"]))
            rc, got, used = run_pairs(st["r"], st["basin"], connectivity, slots)
            want = sc.rows_as_arrays(st["rows"])
            assert rc == 0 and used.tolist() == [len(want[0]), 0], (what, lib().last_error())
            for g, w, column in zip(got, want, ("a", "b", "saddle", "faces")):
                assert np.array_equal(g, w), (what, column)
            for depth in (0.0, 1.0):
                rep, _ = sc.oracle_merge(st["rows"], st["peak_r"], depth)
                set_of_peak = np.full(vol.size, GARBAGE32, dtype=np.int64)      # read at peaks only
                for peak, to in rep.items():
                    set_of_peak[peak] = to
                before = cc.oracle_roots(vol, connectivity).reshape(-1)
                objects = run_relabel(st["basin"], set_of_peak, vol.shape, before)
                expect, _, _ = sc.oracle_separate(vol, connectivity, depth, [value], {value: st})
                assert np.array_equal(objects, expect), (what, depth)
                assert np.array_equal(objects[st["basin"] < 0], before[st["basin"] < 0])      # the other voxels are left alone


def test_a_table_that_is_too_small_is_refused_without_hanging():
    L = lib()
    st = sc.stages_cached("rows_130", 1, 6)
    assert len(st["rows"]) > 8
    for slots in (1, 8):
        rc, _, used = run_pairs(st["r"], st["basin"], 6, slots)
        assert rc == -1 and used[1] == 1 and f"table of {slots} slots is full" in L.last_error()
    rc, _, _ = run_pairs(st["r"], st["basin"], 6, 24)
    assert rc == -1 and "power of two" in L.last_error()
    rc, got, _ = run_pairs(st["r"], st["basin"], 6, 1 << 10)           # the next call works
    assert rc == 0 and len(got[0]) == len(st["rows"])


def test_arguments_are_checked():
    L = lib()
    t = torch.zeros(64, dtype=torch.int32, device=DEV)
    assert L.lib.vs_separate_parents(L.ptr(t), 4, 4, 4, 7, L.ptr(t), L.stream_ptr()) == -1 and "6, 18 or 26" in L.last_error()
    assert L.lib.vs_separate_parents(L.ptr(t), 1 << 31, 1, 1, 6, L.ptr(t), L.stream_ptr()) == -1 and "2^31" in L.last_error()
    assert L.lib.vs_separate_basins(None, 4, 4, 4, L.stream_ptr()) == -1
    assert L.lib.vs_separate_relabel(L.ptr(t), L.ptr(t), 4, 4, 4, L.ptr(t), L.ptr(t), 8, L.stream_ptr()) == -1 and "workspace" in L.last_error()
    assert L.lib.vs_object_moments(L.ptr(t), None, 4, 4, 4, 1, L.ptr(t), L.stream_ptr()) == -1 and "null" in L.last_error()


def test_two_runs_give_the_same_bits():
    st = sc.stages_cached("rows_130", 1, 26)
    slots = sp.table_slots(st["count"], len(st["peak_r"]))
    first, second = run_pairs(st["r"], st["basin"], 26, slots), run_pairs(st["r"], st["basin"], 26, slots)
    assert all(np.array_equal(a, b) for a, b in zip(first[1], second[1]))
    vol = tc.vessels_crop()
    a, b = sp.separate_objects(vol, connectivity=26, device=DEV), sp.separate_objects(vol, connectivity=26, device=DEV)
    assert np.array_equal(a["objects"], b["objects"]) and a["report"] == b["report"]
    assert all(np.array_equal(a["contacts"][k], b["contacts"][k]) for k in a["contacts"])


# ---- the object form of the moments sweep ------------------------------------------------------------------------------------------
def run_moments(vol, ids, row_of_root, rows, by_id):
    L = lib()
    v = torch.from_numpy(np.array(vol).reshape(-1)).to(DEV)
    table = guarded(max(rows, 1) * mc.FIELDS, torch.int64)
    ids_dev, rows_dev = dev32(ids), dev32(row_of_root)
    if by_id:
        L.check(L.lib.vs_object_moments(L.ptr(ids_dev), L.ptr(rows_dev), *vol.shape, rows, L.ptr(table), L.stream_ptr()))
    else:
        L.check(L.lib.vs_component_moments(L.ptr(v), L.ptr(ids_dev), L.ptr(rows_dev), *vol.shape, rows, L.ptr(table), L.stream_ptr()))
    return intact(table).cpu().numpy().reshape(-1, mc.FIELDS)[:rows]


MOMENT_VOLUMES = {"random": lambda: cc.random_labels((17, 33, 65), 4, 0.5, 3), "scene": cc.cleanup_scene, "shells": lambda: cc.shells((19, 21, 135)),
                  "flat": lambda: cc.random_labels((1, 24, 40), 2, 0.5, 4), "stripes": mc.stripes_y, "alternating": mc.alternating_x,
                  "crumbs": lambda: cc.random_labels((9, 10, 67), 4, 0.5, 2), "three_runs": lambda: mc.three_runs((1, 2, 70000)),
                  "solid": lambda: np.full((16, 16, 256), 3, np.uint8), "x63": lambda: cc.random_labels((3, 5, 63), 2, 0.7, 63),
                  "x64": lambda: cc.random_labels((3, 5, 64), 2, 0.7, 64), "x65": lambda: cc.random_labels((3, 5, 65), 2, 0.7, 65),
                  "x257": lambda: cc.random_labels((3, 5, 257), 2, 0.7, 257), "column": lambda: cc.random_labels((7, 1, 5), 2, 0.5, 1),
                  "one": lambda: np.ones((1, 1, 1), np.uint8), "line": lambda: cc.random_labels((1, 1, 37), 4, 0.5, 2)}


@pytest.mark.parametrize("name", sorted(MOMENT_VOLUMES))
def test_object_moments_equal_component_moments_on_component_labellings(name):
    vol = MOMENT_VOLUMES[name]()
    for connectivity, selection in ((6, dict(include_background=True)), (26, dict(min_voxels=2))):
        comp = cc.oracle_roots(vol, connectivity)
        roots, _, row_of_root, _, _ = mc.oracle_selection(vol, comp, **selection)
        by_value, by_id = run_moments(vol, comp, row_of_root, len(roots), False), run_moments(vol, comp, row_of_root, len(roots), True)
        assert np.array_equal(by_id, by_value), (name, connectivity, np.argwhere(by_id != by_value)[:8].tolist())
        assert np.array_equal(by_value, mc.oracle_rows(vol, comp, row_of_root, len(roots))), (name, connectivity)


@pytest.mark.parametrize("name", ["two_balls", "three_balls", "rows_63", "rows_64", "rows_65", "rows_130", "plane", "two_values", "random", "slab_z", "debris_rows"])
def test_object_moments_equal_the_host_table_on_separated_labellings(name):
    vol = sc.scene(name)
    for connectivity, depth in ((6, 0.0), (26, 1.0)):
        objects, _, _ = sc.separate_cached(name, connectivity, depth)
        roots = np.flatnonzero(objects == np.arange(objects.size))
        roots = roots[vol.reshape(-1)[roots] != 0]
        row_of_root = np.full(objects.size, -1, dtype=np.int32)
        row_of_root[roots] = np.arange(len(roots))
        got = run_moments(vol, objects, row_of_root, len(roots), True)
        want = me._table_host(np.asarray(vol), objects, row_of_root, len(roots), by_id=True)
        assert np.array_equal(got, want), (name, connectivity, depth, np.argwhere(got != want)[:8].tolist())


# ---- the Python routes -------------------------------------------------------------------------------------------------------------
def assert_same_separation(got, want, what):
    assert np.array_equal(got["objects"], want["objects"]), what
    assert got["report"] == want["report"], what
    for key in want["contacts"]:
        assert np.array_equal(got["contacts"][key], want["contacts"][key]), (what, key)


@pytest.mark.parametrize("name", sorted(sc.SCENES))
def test_device_route_equals_host_route_and_oracle(name):
    vol = sc.scene(name)
    for connectivity, depth in ((6, 1.0), (18, 0.0), (26, 2.0), (26, float("inf"))):
        values = sc.values_of(vol) + [sc.ABSENT]
        got = sp.separate_objects(vol, values=values, connectivity=connectivity, depth=depth, device=DEV)
        assert_same_separation(got, sp.separate_objects(vol, values=values, connectivity=connectivity, depth=depth, device="cpu"), (name, connectivity, depth))
        assert np.array_equal(got["objects"].reshape(-1), sc.separate_cached(name, connectivity, depth)[0])
        assert got["report"][str(sc.ABSENT)]["separated"] is False
        if depth == float("inf"):
            assert np.array_equal(got["objects"], cc.oracle_roots(vol, connectivity).reshape(vol.shape))


@pytest.mark.parametrize("connectivity", cc.CONNECTIVITIES)
def test_vessels_crop_on_the_device(connectivity):
    vol = tc.vessels_crop()
    expected = sc.vessels_expected()["connectivity"][str(connectivity)]
    dev = torch.from_numpy(vol).to(DEV)
    for depth in sc.DEPTHS:
        got = sp.separate_objects(dev, values=[255], connectivity=connectivity, depth=depth)      # a device tensor chooses the device
        assert_same_separation(got, sp.separate_objects(vol, values=[255], connectivity=connectivity, depth=depth, device="cpu"), (connectivity, depth))
        report, want = got["report"]["255"], expected["objects"][str(depth)]
        assert (report["basins"], report["pair_rows"], report["adjacent_pairs"]) == (expected["basins"], expected["pair_rows"], expected["adjacent_pairs"])
        assert (report["objects"], report["merges"], len(got["contacts"]["root_a"])) == (want["count"], want["merges"], want["contacts"])
        roots, sizes = np.unique(got["objects"][vol == 255], return_counts=True)
        assert roots.tolist() == want["roots"] and sizes.tolist() == want["voxels"]
    separate = dict(values=[255], depth=1.0, max_pairs=sp.DEFAULT_MAX_PAIRS)
    mc.assert_raw_equal(me.measure_components(dev, connectivity=connectivity, min_voxels=2, separate=separate),
                        me.measure_components(vol, connectivity=connectivity, min_voxels=2, separate=separate, device="cpu"), connectivity)
    assert np.array_equal(me.object_ids(dev, connectivity=connectivity, separate=separate), me.object_ids(vol, connectivity=connectivity, separate=separate, device="cpu"))
    with pytest.raises(ValueError, match=f"has {expected['pair_rows']} rows, more than measure_separate_max_pairs = 50"):
        sp.separate_objects(dev, values=[255], connectivity=connectivity, max_pairs=50)


# ---- the manager and the command ---------------------------------------------------------------------------------------------------
def test_manager_and_command_with_the_keys(golden, tmp_path):
    from oracle.unet_resnet34_torch import seeded_oracle
    from volume_segmantics_amd.checkpoint_compat import reference_pickle_enum
    from volume_segmantics_amd.model.operations.vol_seg_prediction_manager import VolSeg2DPredictionManager
    from volume_segmantics_amd.scripts import measure_2d_prediction
    from volume_segmantics_amd.utilities import base_data_utils as utils
    vol = golden("g3_predict_29x64x40_c4.npz")["vol"]
    path = tmp_path / "model.pytorch"
    torch.save({"model_state_dict": seeded_oracle(4, 0).state_dict(),
                "model_struc_dict": {"type": reference_pickle_enum(utils.ModelType.U_NET), "encoder_name": "resnet34",
                                     "encoder_weights": "imagenet", "in_channels": 1, "classes": 4},
                "optimizer_state_dict": {}, "loss_val": 0.1, "label_codes": {"fg": 1}}, path)
    settings = SimpleNamespace(quality="low", output_probs=False, clip_data=False, st_dev_factor=2.575, data_hdf5_path="/data",
                               cuda_device=0, downsample=False, one_hot=False, prediction_axis="Z", prediction_batch_size=7,
                               measure_objects=True, measure_min_voxels=2, measure_voxel_size=[2.0, 1.0, 1.0], measure_save_ids=True)
    manager = VolSeg2DPredictionManager(str(path), vol, settings)
    for name in ("plain", "apart"):
        (tmp_path / name).mkdir()
    plain = manager.predict_volume_to_path(tmp_path / "plain" / "seg.npy")
    assert "separation" not in manager.last_measurements
    assert sorted(p.name for p in (tmp_path / "plain").iterdir()) == ["seg.npy", "seg_object_ids.h5", "seg_objects.csv", "seg_objects.json"]

    settings.measure_separate, settings.measure_separate_depth = True, 0.5
    same = manager.predict_volume_to_path(tmp_path / "apart" / "seg.npy")
    assert np.array_equal(same, plain)
    assert sorted(p.name for p in (tmp_path / "apart").iterdir()) == ["seg.npy", "seg_object_contacts.csv", "seg_object_contacts.json", "seg_object_ids.h5",
                                                                      "seg_objects.csv", "seg_objects.json"]
    want = me.measure_label_volume(plain, settings, device="cpu")
    kept = manager.last_measurements
    mc.assert_raw_equal(kept["raw"], want["raw"])
    assert np.array_equal(kept["ids"], want["ids"]) and kept["separation"]["report"] == want["separation"]["report"]
    for column in sp.CONTACT_COLUMNS:
        assert kept["separation"]["contacts"][column].tobytes() == want["separation"]["contacts"][column].tobytes(), column
    assert len(kept["raw"]["roots"]) >= len(me.measure_components(plain, min_voxels=2, device="cpu")["roots"])
    doc = json.loads((tmp_path / "apart" / "seg_objects.json").read_text())
    assert doc["separation"]["settings"]["depth"] == 0.5 and doc["separation"]["report"] == want["separation"]["report"]
    mc.assert_raw_equal(me.raw_from_json(doc), want["raw"])
    assert np.array_equal(utils.numpy_from_hdf5(tmp_path / "apart" / "seg_object_ids.h5")[0], want["ids"])

    (tmp_path / "volseg-settings").mkdir()
    (tmp_path / "volseg-settings" / "2d_model_predict_settings.yaml").write_text(
        "measure_min_voxels: 2\nmeasure_voxel_size: [2.0, 1.0, 1.0]\nmeasure_separate: true\nmeasure_separate_depth: 0.5\n")
    utils.save_data_to_hdf5(plain, tmp_path / "pred.h5")
    measure_2d_prediction.main([str(tmp_path / "pred.h5"), "--data_dir", str(tmp_path)])
    assert (tmp_path / "pred_object_contacts.csv").read_text() == (tmp_path / "apart" / "seg_object_contacts.csv").read_text()
    mc.assert_raw_equal(me.raw_from_json(json.loads((tmp_path / "pred_objects.json").read_text())), want["raw"])
