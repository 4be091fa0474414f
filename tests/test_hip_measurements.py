"""-m gpu: vs_component_moments (csrc/measure.hip) through the C ABI, integer for integer against the per-component oracle of
tests/measurement_cases.py at every size where the kernel takes another path - rows that straddle the 4-byte loads and the
64-voxel sub-steps, one row taking every contribution, runs of length 1, more rows per sub-step than ballot rounds, more rows per
span than cache slots, rows that are not measured, sums beyond 2^32 - then the Python route on the device against the host route,
the committed vessels integers, and VolSeg2DPredictionManager with the measure keys.  The table starts out full of garbage; nothing
here has a tolerance."""
import json
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import components_cases as cc
import measurement_cases as mc
from hip_helpers import DEV, lib
from volume_segmantics_amd.utilities import measurements as me

pytestmark = pytest.mark.gpu

GARBAGE64 = -0x0123456789ABCDEF


# ---- the kernel through the C ABI --------------------------------------------------------------------------------------------------
def run_moments(vol, comp, row_of_root, rows):
    L = lib()
    z, y, x = vol.shape
    v = torch.from_numpy(np.array(vol).reshape(-1)).to(DEV)
    c = torch.from_numpy(np.ascontiguousarray(comp).reshape(-1).astype(np.int32)).to(DEV)
    r = torch.from_numpy(np.ascontiguousarray(row_of_root).reshape(-1).astype(np.int32)).to(DEV)
    table = torch.full((max(rows, 1), mc.FIELDS), GARBAGE64, dtype=torch.int64, device=DEV)
    L.check(L.lib.vs_component_moments(L.ptr(v), L.ptr(c), L.ptr(r), z, y, x, rows, L.ptr(table), L.stream_ptr()))
    torch.cuda.synchronize()
    return table.cpu().numpy()[:rows]


def assert_moments(vol, connectivity=6, **selection):
    """every component measured (background included) unless `selection` says otherwise"""
    selection = selection or dict(include_background=True)
    comp = cc.oracle_roots(vol, connectivity)
    roots, _, row_of_root, _, _ = mc.oracle_selection(vol, comp, **selection)
    got, want = run_moments(vol, comp, row_of_root, len(roots)), mc.oracle_rows(vol, comp, row_of_root, len(roots))
    assert np.array_equal(got, want), (vol.shape, connectivity, np.argwhere(got != want)[:8].tolist(), got[got != want][:8], want[got != want][:8])
    return got


@pytest.mark.parametrize("shape", mc.DEGENERATE_SHAPES)
def test_degenerate_shapes(shape):
    for k, seed in ((2, 1), (4, 2)):
        for c in cc.CONNECTIVITIES:
            assert_moments(cc.random_labels(shape, k, 0.5, seed), c)
    assert_moments(np.full(shape, 7, np.uint8))


@pytest.mark.parametrize("x", [63, 64, 65, 257])
def test_rows_that_straddle_loads_and_sub_steps(x):
    vol = cc.random_labels((3, 5, x), 2, 0.7, x)
    vol[0, 0, :] = 1                                                # one run along a whole row
    vol[1, 2, 5:x - 3] = 0
    assert_moments(vol)
    assert_moments(vol, 26)


def test_one_solid_component_takes_every_contribution():
    shape = (16, 16, 256)
    got = assert_moments(np.full(shape, 3, np.uint8))
    n = 16 * 16 * 256
    assert got[0, 0] == n and got[0, 16:20].tolist() == [2 * 16 * 256, 2 * 16 * 256, 2 * 16 * 16, 1]
    assert got[0, 6] == 16 * 16 * sum(i * i for i in range(256))


def test_runs_of_length_one():
    got = assert_moments(mc.alternating_x((4, 8, 130)))
    assert got.shape == (2, 20) and got[:, 0].tolist() == [4 * 8 * 65] * 2


def test_more_rows_per_sub_step_than_ballot_rounds():
    vol = cc.random_labels((9, 10, 67), 4, 0.5, 2)
    got = assert_moments(vol, 6)
    assert len(got) > 1000


def test_more_rows_per_span_than_cache_slots():
    got = assert_moments(mc.stripes_y((2, 80, 70), 40), include_background=False)
    assert got.shape == (40, 20) and (got[:, 0] == 2 * 2 * 70).all()


def test_measured_and_unmeasured_rows():
    vol = cc.random_labels((9, 10, 67), 4, 0.5, 5)
    assert_moments(vol, 26, min_voxels=4)                           # the background and the crumbs are -1
    assert_moments(vol, 18, min_voxels=2, include_background=True)
    comp = cc.oracle_roots(vol, 26)
    roots, _, row_of_root, _, _ = mc.oracle_selection(vol, comp, include_background=True)
    spread = np.where(row_of_root >= 0, row_of_root * 2 + 1, -1)    # rows nothing maps to: 0 voxels and the empty box
    got = run_moments(vol, comp, spread, 2 * len(roots) + 1)
    assert np.array_equal(got, mc.oracle_rows(vol, comp, spread, 2 * len(roots) + 1))
    assert got[0].tolist() == [0] * 10 + [9, -1, 10, -1, 67, -1] + [0] * 4


def test_no_rows_and_errors():
    L = lib()
    vol = cc.random_labels((5, 7, 9), 4, 0.5, 8)
    comp = cc.oracle_roots(vol, 6)
    nothing = np.full(vol.size, -1, dtype=np.int32)
    assert run_moments(vol, comp, nothing, 0).shape == (0, 20)
    assert L.lib.vs_component_moments(None, None, None, 5, 7, 9, 0, None, L.stream_ptr()) == 0      # no launch: nothing is touched
    v = torch.from_numpy(vol.reshape(-1)).to(DEV)
    c = torch.from_numpy(comp.reshape(-1).astype(np.int32)).to(DEV)
    table = torch.zeros((4, 20), dtype=torch.int64, device=DEV)
    for extents in ((1 << 31, 1, 1), (2048, 1024, 1024), (0, 4, 4)):
        rc = L.lib.vs_component_moments(L.ptr(v), L.ptr(c), L.ptr(c), *extents, 4, L.ptr(table), L.stream_ptr())
        assert rc == -1 and "2^31" in L.last_error(), extents
    rc = L.lib.vs_component_moments(L.ptr(v), L.ptr(c), None, 5, 7, 9, 4, L.ptr(table), L.stream_ptr())
    assert rc == -1 and "null" in L.last_error()
    rc = L.lib.vs_component_moments(L.ptr(v), L.ptr(c), L.ptr(c), 5, 7, 9, -1, L.ptr(table), L.stream_ptr())
    assert rc == -1 and "rows" in L.last_error()
    assert_moments(vol)                                             # the next call works


def test_sums_beyond_32_bits_and_closed_forms_at_large_x():
    got = assert_moments(mc.three_runs((1, 2, 70000)), include_background=False)
    assert got.shape == (3, 20) and got[2, 6] == 2 * sum(i * i for i in range(65536, 70000)) > 2 ** 32
    assert got[:, 18].tolist() == [4, 4, 4] and got[:, 16].tolist() == [0, 0, 0] and got[:, 17].tolist() == [40000, 2 * 45536, 2 * 4464]


# ---- device route against host route ---------------------------------------------------------------------------------------------
ROUTE_VOLUMES = {"random": lambda: cc.random_labels((17, 33, 65), 4, 0.5, 3), "scene": cc.cleanup_scene, "shells": lambda: cc.shells((19, 21, 135)),
                 "flat": lambda: cc.random_labels((1, 24, 40), 2, 0.5, 4), "stripes": mc.stripes_y}


@pytest.mark.parametrize("name", sorted(ROUTE_VOLUMES))
def test_device_route_equals_host_route(name):
    vol = ROUTE_VOLUMES[name]()
    for c, kw in ((6, dict()), (18, dict(min_voxels=3, include_background=True)), (26, dict(min_voxels=2))):
        got, want = me.measure_components(vol, connectivity=c, device=DEV, **kw), me.measure_components(vol, connectivity=c, device="cpu", **kw)
        mc.assert_raw_equal(got, want, (name, c))
        a, b = me.object_table(got, [2.0, 1.0, 0.5]), me.object_table(want, [2.0, 1.0, 0.5])
        assert a["summary"] == b["summary"] or json.dumps(a["summary"]) == json.dumps(b["summary"])
        for column in me.COLUMNS:
            assert a["objects"][column].tobytes() == b["objects"][column].tobytes(), (name, c, column)      # bit for bit
        assert np.array_equal(me.object_ids(vol, connectivity=c, device=DEV, **kw), me.object_ids(vol, connectivity=c, device="cpu", **kw))
    mc.assert_raw_equal(me.measure_components(vol, connectivity=6, device=DEV), mc.oracle_measure(vol, 6), name)


def test_device_route_takes_tensors_and_unaligned_views():
    vol = cc.cleanup_scene()
    want = me.measure_components(vol, 18, device="cpu")
    dev = torch.from_numpy(np.array(vol)).to(DEV)
    mc.assert_raw_equal(me.measure_components(dev, 18), want)       # a device tensor chooses the device
    mc.assert_raw_equal(me.measure_components(dev.to(torch.int64), 18), want)
    view = torch.from_numpy(np.concatenate([np.zeros(3, np.uint8), vol.reshape(-1)])).to(DEV)[3:].reshape(vol.shape)
    assert view.data_ptr() % 16 != 0
    mc.assert_raw_equal(me.measure_components(view, 18), want)
    ids = me.object_ids(dev, 18)
    assert ids.dtype == np.int32 and np.array_equal(ids, me.object_ids(vol, 18, device="cpu"))


def test_too_little_device_memory_is_a_value_error(monkeypatch):
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda device=None: (1000, 1 << 30))
    with pytest.raises(ValueError, match=r"needs \d+ bytes of device memory but only 1000 bytes are free"):
        me.measure_components(cc.cleanup_scene(), device=DEV)


@pytest.mark.parametrize("connectivity", [6, 26])
def test_vessels_fixture_against_the_committed_integers(connectivity):
    expected = mc.vessels_expected()[str(connectivity)]
    dev = torch.from_numpy(np.array(cc.vessels())).to(DEV)
    raw = me.measure_components(dev, connectivity=connectivity, include_background=True)
    assert raw["roots"].tolist() == expected["roots"] and raw["values"].tolist() == expected["values"]
    assert raw["table"].tolist() == expected["table"] and not raw["not_listed_objects"].any()
    again = me.measure_components(dev, connectivity=connectivity, include_background=True)
    assert np.array_equal(again["table"], raw["table"])             # the same bits on a second call


# ---- the manager -------------------------------------------------------------------------------------------------------------------
def test_manager_measures_the_saved_volume(golden, tmp_path):
    from oracle.unet_resnet34_torch import seeded_oracle
    from volume_segmantics_amd.checkpoint_compat import reference_pickle_enum
    from volume_segmantics_amd.model.operations.vol_seg_prediction_manager import VolSeg2DPredictionManager
    from volume_segmantics_amd.utilities.base_data_utils import ModelType, numpy_from_hdf5
    vol = golden("g3_predict_29x64x40_c4.npz")["vol"]
    path = tmp_path / "model.pytorch"
    torch.save({"model_state_dict": seeded_oracle(4, 0).state_dict(),
                "model_struc_dict": {"type": reference_pickle_enum(ModelType.U_NET), "encoder_name": "resnet34",
                                     "encoder_weights": "imagenet", "in_channels": 1, "classes": 4},
                "optimizer_state_dict": {}, "loss_val": 0.1, "label_codes": {"fg": 1}}, path)
    settings = SimpleNamespace(quality="low", output_probs=False, clip_data=False, st_dev_factor=2.575, data_hdf5_path="/data",
                               cuda_device=0, downsample=False, one_hot=False, prediction_axis="Z", prediction_batch_size=7)
    manager = VolSeg2DPredictionManager(str(path), vol, settings)
    for name in ("absent", "again", "on", "cleaned"):
        (tmp_path / name).mkdir()

    raw = manager.predict_volume_to_path(tmp_path / "absent" / "seg.npy")
    assert manager.last_measurements is None
    manager.predict_volume_to_path(tmp_path / "again" / "seg.npy")
    assert (tmp_path / "again" / "seg.npy").read_bytes() == (tmp_path / "absent" / "seg.npy").read_bytes()
    assert [p.name for p in (tmp_path / "absent").iterdir()] == ["seg.npy"]

    settings.measure_objects = True
    settings.measure_min_voxels = 2
    settings.measure_voxel_size = [2.0, 1.0, 1.0]
    settings.measure_save_ids = True
    same = manager.predict_volume_to_path(tmp_path / "on" / "seg.npy")
    assert np.array_equal(same, raw) and (tmp_path / "on" / "seg.npy").read_bytes() == (tmp_path / "absent" / "seg.npy").read_bytes()
    assert sorted(p.name for p in (tmp_path / "on").iterdir()) == ["seg.npy", "seg_object_ids.h5", "seg_objects.csv", "seg_objects.json"]
    saved = np.load(tmp_path / "on" / "seg.npy")
    want = me.measure_components(saved, connectivity=6, min_voxels=2, device="cpu")
    doc = json.loads((tmp_path / "on" / "seg_objects.json").read_text())
    assert len(doc["objects"]) == len(want["roots"]) > 0 and doc["settings"]["min_voxels"] == 2 and doc["voxel_size"] == [2.0, 1.0, 1.0]
    mc.assert_raw_equal(me.raw_from_json(doc), want)
    mc.assert_raw_equal(manager.last_measurements["raw"], want)
    ids = numpy_from_hdf5(tmp_path / "on" / "seg_object_ids.h5")[0]
    assert np.array_equal(ids, me.object_ids(saved, connectivity=6, min_voxels=2, device="cpu")) and np.array_equal(ids, manager.last_measurements["ids"])

    settings.measure_save_ids = False
    settings.postprocess_min_object_size = 6                        # the measured volume is the cleaned one, under its connectivity
    settings.postprocess_connectivity = 26
    cleaned = manager.predict_volume_to_path(tmp_path / "cleaned" / "seg.npy")
    assert not np.array_equal(cleaned, raw) and np.array_equal(manager.last_postprocess["raw"], raw)
    want = me.measure_components(cleaned, connectivity=26, min_voxels=2, device="cpu")
    mc.assert_raw_equal(manager.last_measurements["raw"], want)
    assert want["table"][:, 0].min() >= 6 and manager.last_measurements["settings"]["connectivity"] == 26
    mc.assert_raw_equal(me.raw_from_json(json.loads((tmp_path / "cleaned" / "seg_objects.json").read_text())), want)
    assert not (tmp_path / "cleaned" / "seg_object_ids.h5").exists()

    settings.one_hot = True
    with pytest.raises(ValueError, match="one_hot"):
        manager.predict_volume_to_path(None)
