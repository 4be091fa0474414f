"""-m gpu: vs_mesh_count and vs_mesh_emit (csrc/mesh.hip) through the C ABI, bit for bit against the cell-by-cell oracle of
tests/mesh_cases.py in both styles at every size where the kernels take another path - degenerate extents, rows of cells that end
before, on and after a 64-cell chunk, long stretches of empty chunks, every cell active, an absent value, more chunks than one
workgroup of the scan covers - then determinism, the Python route on the device against the host route, the committed vessels
figures, and VolSeg2DPredictionManager with the mesh keys.  Outputs start out full of garbage; nothing here has a tolerance."""
import json
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import components_cases as cc
import mesh_cases as mc
from hip_helpers import DEV, lib
from volume_segmantics_amd.utilities import meshes as me

pytestmark = pytest.mark.gpu

GARBAGE64 = -0x0123456789ABCDEF
GARBAGE32 = -0x01234567
STYLE = {"smooth": 0, "blocky": 1}                      # include/volseg_hip.h VS_MESH_SMOOTH / VS_MESH_BLOCKY
# csrc/mesh.hip: kThreads x kScanItems words are one workgroup's tile of the scan (kScanTile); a chunk is 64 cells of a row of cells
K_THREADS, K_SCAN_ITEMS, CHUNK = 256, 4, 64
K_SCAN_TILE = K_THREADS * K_SCAN_ITEMS
K_TOTAL_SLOTS = 256                                     # kTotalSlots: partial totals of 4 words each at the workspace's end


def chunks_of(shape):
    z, y, x = shape
    return (z + 1) * (y + 1) * ((x + 1 + CHUNK - 1) // CHUNK)


# ---- the kernels through the C ABI -------------------------------------------------------------------------------------------------
def run_count(v, shape, value):
    L = lib()
    need = L.lib.vs_mesh_workspace_bytes(*shape)
    level1 = -(-chunks_of(shape) // K_SCAN_TILE)
    assert need == 8 * (2 * chunks_of(shape) + level1 + -(-level1 // K_SCAN_TILE) + 4 * K_TOTAL_SLOTS)
    work = torch.full((need,), 0xA5, dtype=torch.uint8, device=DEV)
    totals = torch.full((4,), GARBAGE64, dtype=torch.int64, device=DEV)
    L.check(L.lib.vs_mesh_count(L.ptr(v), *shape, value, L.ptr(work), need, L.ptr(totals), L.stream_ptr()))
    torch.cuda.synchronize()
    return work, totals.cpu().tolist()


def run_emit(v, shape, value, style, work, totals):
    """(vertices, quads) with one row of garbage kept behind each: it must stay"""
    L = lib()
    n_vertices, n_quads = totals[0], sum(totals[1:])
    vertices = torch.full((n_vertices + 1, 3), float("nan"), dtype=torch.float32, device=DEV)
    quads = torch.full((n_quads + 1, 4), GARBAGE32, dtype=torch.int32, device=DEV)
    nothing = n_vertices == 0 and n_quads == 0
    L.check(L.lib.vs_mesh_emit(L.ptr(v), *shape, value, STYLE[style], L.ptr(work), work.numel(), None if nothing else L.ptr(vertices),
                               None if nothing else L.ptr(quads), L.stream_ptr()))
    torch.cuda.synchronize()
    vertices, quads = vertices.cpu().numpy(), quads.cpu().numpy()
    assert np.isnan(vertices[-1]).all() and (quads[-1] == GARBAGE32).all()           # nothing else is touched
    return vertices[:-1], quads[:-1]


def run_mesh(vol, value, style):
    shape = tuple(vol.shape)
    v = torch.from_numpy(np.array(vol).reshape(-1)).to(DEV)
    work, totals = run_count(v, shape, value)
    vertices, quads = run_emit(v, shape, value, style, work, totals)
    return vertices, quads, totals[1:]


def assert_mesh(vol, value, want=None):
    for style in mc.STYLES:
        mc.assert_mesh_equal(run_mesh(vol, value, style), mc.oracle_mesh(vol, value, style) if want is None else want[style], (vol.shape, value, style))


@pytest.mark.parametrize("name", sorted(mc.VOLUMES))
def test_named_volumes_against_the_oracle(name):
    """the degenerate extents, the solid box, the through hole, the shell, the edge pair, the checkerboard (every cell active, 3 quads
    per interior owner), random labels with K = 2 and 4, and M touching every face of the volume"""
    vol = mc.VOLUMES[name]()
    for value in sorted(set(np.unique(vol).tolist()) | {0}):
        assert_mesh(vol, value, {style: mc.oracle_cached(name, value, style) for style in mc.STYLES})


@pytest.mark.parametrize("x", [62, 63, 64, 65, 127, 128, 129])
def test_rows_that_end_before_on_and_after_a_chunk(x):
    """the X + 1 cells of a row; a run of M along a whole row and one that stops 3 cells short"""
    vol = mc.row_runs(x)
    assert_mesh(vol, 1)
    assert_mesh(vol, 0)


@pytest.mark.parametrize("y", [6, 7, 8, 15, 16])
def test_rows_of_cells_that_end_before_on_and_after_a_column(y):
    """a wave takes kRowsPerWave = 8 rows of cells: the Y + 1 rows end one short of, on and one past a multiple of it"""
    vol = cc.random_labels((3, y, 70), 2, 0.5, y)
    assert_mesh(vol, 1)


def test_solid_volume_has_only_border_cells():
    vol = np.full((6, 7, 200), 5, np.uint8)
    for style in mc.STYLES:
        vertices, quads, per_axis = run_mesh(vol, 5, style)
        assert per_axis == [2 * 7 * 200, 2 * 6 * 200, 2 * 6 * 7] and len(vertices) == 7 * 8 * 201 - 5 * 6 * 199
        mc.assert_mesh_equal((vertices, quads, per_axis), mc.oracle_mesh(vol, 5, style), style)


def test_absent_value_gives_nothing():
    vol = cc.random_labels((5, 7, 70), 4, 0.5, 8)
    v = torch.from_numpy(vol.reshape(-1)).to(DEV)
    work, totals = run_count(v, vol.shape, 9)
    assert totals == [0, 0, 0, 0]
    vertices, quads = run_emit(v, vol.shape, 9, "smooth", work, totals)
    assert vertices.shape == (0, 3) and quads.shape == (0, 4)


def test_more_chunks_than_one_workgroup_of_the_scan_covers():
    """more than kScanTile chunks: the first scan level runs with several workgroups and the level above it runs at all"""
    shape = (10, 31, 129)
    assert K_SCAN_TILE < chunks_of(shape) < 2 * K_SCAN_TILE + 64
    vol = cc.random_labels(shape, 2, 0.3, 21)
    assert_mesh(vol, 1)


def test_three_scan_levels_against_the_host_route():
    """more than kScanTile^2 chunks, so that the second level runs with several workgroups and the third runs: too many cells for the
    cell-by-cell oracle, so the arrays are held to the host route, which tests/test_meshes_host.py holds to the oracle"""
    shape = (1024, 1024, 1)
    assert chunks_of(shape) > K_SCAN_TILE ** 2
    vol = cc.random_labels(shape, 2, 0.4, 22)
    want = me.extract_surface(vol, 1, "smooth", device="cpu")
    mc.assert_mesh_equal(run_mesh(vol, 1, "smooth"), want, shape)


def test_count_twice_and_emit_twice_give_equal_bytes():
    vol = cc.random_labels((9, 10, 135), 4, 0.5, 5)
    v = torch.from_numpy(vol.reshape(-1)).to(DEV)
    first, totals = run_count(v, vol.shape, 2)
    second, again = run_count(v, vol.shape, 2)
    assert totals == again and torch.equal(first, second)
    for style in mc.STYLES:
        a, b = run_emit(v, vol.shape, 2, style, first, totals), run_emit(v, vol.shape, 2, style, second, totals)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    mc.assert_mesh_equal((a[0], a[1], totals[1:]), mc.oracle_mesh(vol, 2, "blocky"))


def test_errors():
    L = lib()
    vol = cc.random_labels((5, 7, 9), 4, 0.5, 8)
    v = torch.from_numpy(vol.reshape(-1)).to(DEV)
    work, totals = run_count(v, vol.shape, 1)
    out = torch.zeros(64, dtype=torch.int64, device=DEV)
    for extents in ((1289, 1289, 1290), (1 << 31, 1, 1), (0, 4, 4)):
        assert L.lib.vs_mesh_workspace_bytes(*extents) == 0
        rc = L.lib.vs_mesh_count(L.ptr(v), *extents, 1, L.ptr(work), work.numel(), L.ptr(out), L.stream_ptr())
        assert rc == -1 and "2^31" in L.last_error(), extents
        rc = L.lib.vs_mesh_emit(L.ptr(v), *extents, 1, 0, L.ptr(work), work.numel(), L.ptr(out), L.ptr(out), L.stream_ptr())
        assert rc == -1 and "2^31" in L.last_error(), extents
    assert L.lib.vs_mesh_count(L.ptr(v), 5, 7, 9, 256, L.ptr(work), work.numel(), L.ptr(out), L.stream_ptr()) == -1 and "uint8" in L.last_error()
    assert L.lib.vs_mesh_count(L.ptr(v), 5, 7, 9, 1, L.ptr(work), work.numel() - 8, L.ptr(out), L.stream_ptr()) == -1 and "workspace" in L.last_error()
    assert L.lib.vs_mesh_count(L.ptr(v), 5, 7, 9, 1, None, work.numel(), L.ptr(out), L.stream_ptr()) == -1 and "null" in L.last_error()
    assert L.lib.vs_mesh_emit(L.ptr(v), 5, 7, 9, 1, 2, L.ptr(work), work.numel(), L.ptr(out), L.ptr(out), L.stream_ptr()) == -1 and "style" in L.last_error()
    assert L.lib.vs_mesh_emit(L.ptr(v), 5, 7, 9, 1, 0, L.ptr(work), work.numel(), L.ptr(out), None, L.stream_ptr()) == -1 and "null" in L.last_error()
    assert L.lib.vs_mesh_emit(None, 5, 7, 9, 1, 0, L.ptr(work), work.numel(), None, None, L.stream_ptr()) == 0        # nothing to emit: no launch
    mc.assert_mesh_equal((*run_emit(v, vol.shape, 1, "smooth", work, totals), totals[1:]), mc.oracle_mesh(vol, 1, "smooth"))      # the next call works


# ---- device route against host route ---------------------------------------------------------------------------------------------
ROUTE_VOLUMES = {"random": lambda: cc.random_labels((17, 33, 65), 4, 0.5, 3), "scene": cc.cleanup_scene, "shells": lambda: cc.shells((19, 21, 135)),
                 "flat": lambda: cc.random_labels((1, 24, 40), 2, 0.5, 4), "checkerboard": cc.checkerboard}


@pytest.mark.parametrize("name", sorted(ROUTE_VOLUMES))
def test_device_route_equals_host_route(name):
    vol = ROUTE_VOLUMES[name]()
    for value in np.unique(vol).tolist():
        for style in mc.STYLES:
            got, want = me.extract_surface(vol, value, style, device=DEV), me.extract_surface(vol, value, style, device="cpu")
            mc.assert_mesh_equal(got, want, (name, value, style))
            assert got["shape"].tolist() == want["shape"].tolist()
            assert json.dumps(me.mesh_summary(got, [2.0, 1.0, 0.5])) == json.dumps(me.mesh_summary(want, [2.0, 1.0, 0.5]))      # bit for bit: repr of every float
    dev = torch.from_numpy(np.array(vol)).to(DEV)
    settings = SimpleNamespace(mesh_style="blocky")
    a, b = me.mesh_label_volume(dev, settings), me.mesh_label_volume(vol, settings, device="cpu")     # a device tensor chooses the device
    assert list(a["surfaces"]) == list(b["surfaces"]) == [v for v in np.unique(vol).tolist() if v != 0] and a["summary"] == b["summary"]


def test_device_route_takes_unaligned_views_and_wide_labels():
    vol = cc.cleanup_scene()
    want = me.extract_surface(vol, 1, device="cpu")
    dev = torch.from_numpy(np.array(vol)).to(DEV)
    mc.assert_mesh_equal(me.extract_surface(dev.to(torch.int64), 1), want)
    view = torch.from_numpy(np.concatenate([np.zeros(3, np.uint8), vol.reshape(-1)])).to(DEV)[3:].reshape(vol.shape)
    assert view.data_ptr() % 16 != 0
    mc.assert_mesh_equal(me.extract_surface(view, 1), want)


def test_too_little_device_memory_is_a_value_error(monkeypatch):
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda device=None: (1000, 1 << 30))
    with pytest.raises(ValueError, match=r"needs \d+ bytes of device memory but only 1000 bytes are free"):
        me.extract_surface(cc.cleanup_scene(), 1, device=DEV)


@pytest.mark.parametrize("style", mc.STYLES)
def test_vessels_fixture_against_the_committed_figures(style):
    dev = torch.from_numpy(np.array(cc.vessels())).to(DEV)
    for value, per_style in mc.vessels_expected().items():
        s = me.extract_surface(dev, int(value), style)
        want = per_style[style]
        assert len(s["vertices"]) == want["vertices"] and s["quads_per_axis"].tolist() == want["quads_per_axis"] and mc.digest(s) == want["sha256"]


def test_mesh_command_on_the_vessels_labels(tmp_path):
    """the PLY the command writes from the vessels volume has the header counts of the committed figures"""
    from volume_segmantics_amd.scripts import mesh_2d_prediction
    mesh_2d_prediction.main([str(mc.GOLDEN / "vessels_256cube_LABELS.h5"), "--data_dir", str(tmp_path), "--output", str(tmp_path / "vessels")])
    want = mc.vessels_expected()["255"]["smooth"]
    lines = (tmp_path / "vessels_mesh_255.ply").read_bytes()[:400].decode("ascii", "replace").splitlines()
    assert f"element vertex {want['vertices']}" in lines and f"element face {sum(want['quads_per_axis'])}" in lines
    doc = json.loads((tmp_path / "vessels_meshes.json").read_text())
    assert doc["meshes"]["255"]["closed"] is True and [doc["meshes"]["255"]["quads_" + a] for a in "zyx"] == want["quads_per_axis"]


# ---- the manager -------------------------------------------------------------------------------------------------------------------
def test_manager_meshes_the_saved_volume(golden, tmp_path):
    from oracle.unet_resnet34_torch import seeded_oracle
    from volume_segmantics_amd.checkpoint_compat import reference_pickle_enum
    from volume_segmantics_amd.model.operations.vol_seg_prediction_manager import VolSeg2DPredictionManager
    from volume_segmantics_amd.utilities.base_data_utils import ModelType
    vol = golden("g3_predict_29x64x40_c4.npz")["vol"]
    path = tmp_path / "model.pytorch"
    torch.save({"model_state_dict": seeded_oracle(4, 0).state_dict(),
                "model_struc_dict": {"type": reference_pickle_enum(ModelType.U_NET), "encoder_name": "resnet34",
                                     "encoder_weights": "imagenet", "in_channels": 1, "classes": 4},
                "optimizer_state_dict": {}, "loss_val": 0.1, "label_codes": {"fg": 1}}, path)
    settings = SimpleNamespace(quality="low", output_probs=False, clip_data=False, st_dev_factor=2.575, data_hdf5_path="/data",
                               cuda_device=0, downsample=False, one_hot=False, prediction_axis="Z", prediction_batch_size=7)
    manager = VolSeg2DPredictionManager(str(path), vol, settings)
    for name in ("absent", "on", "stl"):
        (tmp_path / name).mkdir()

    raw = manager.predict_volume_to_path(tmp_path / "absent" / "seg.npy")
    assert manager.last_meshes is None and [p.name for p in (tmp_path / "absent").iterdir()] == ["seg.npy"]

    settings.mesh_surfaces = True
    settings.mesh_voxel_size = [2.0, 1.0, 1.0]
    same = manager.predict_volume_to_path(tmp_path / "on" / "seg.npy")
    assert np.array_equal(same, raw) and (tmp_path / "on" / "seg.npy").read_bytes() == (tmp_path / "absent" / "seg.npy").read_bytes()
    values = [v for v in np.unique(raw).tolist() if v != 0]
    assert len(values) >= 1
    assert sorted(p.name for p in (tmp_path / "on").iterdir()) == sorted(["seg.npy", "seg_meshes.json"] + [f"seg_mesh_{v}.ply" for v in values])
    doc = json.loads((tmp_path / "on" / "seg_meshes.json").read_text())
    assert list(doc["meshes"]) == [str(v) for v in values] and doc["settings"]["voxel_size"] == [2.0, 1.0, 1.0]
    for value in values:
        want = me.extract_surface(raw, value, "smooth", device="cpu")
        mc.assert_mesh_equal(manager.last_meshes["surfaces"][value], want, value)
        assert json.dumps(manager.last_meshes["summary"][str(value)]) == json.dumps(me.mesh_summary(want, [2.0, 1.0, 1.0]))
        lines, vertices, faces, _ = mc.read_ply(tmp_path / "on" / f"seg_mesh_{value}.ply")
        assert len(vertices) == len(want["vertices"]) and faces[0] == want["quads"][0].tolist() and faces[-1] == want["quads"][-1].tolist()
        assert doc["meshes"][str(value)]["closed"] is True

    settings.mesh_format, settings.mesh_values, settings.mesh_style = "stl", [values[0]], "blocky"
    settings.postprocess_min_object_size = 6                        # the meshed volume is the cleaned one
    cleaned = manager.predict_volume_to_path(tmp_path / "stl" / "seg.npy")
    assert sorted(p.name for p in (tmp_path / "stl").iterdir()) == sorted(["seg.npy", "seg_components.csv", "seg_components.json", "seg_meshes.json",
                                                                           f"seg_mesh_{values[0]}.stl"])
    mc.assert_mesh_equal(manager.last_meshes["surfaces"][values[0]], me.extract_surface(cleaned, values[0], "blocky", device="cpu"))
    assert manager.last_meshes["summary"][str(values[0])]["enclosed_volume"] == 2.0 * int((cleaned == values[0]).sum())

    settings.one_hot = True
    with pytest.raises(ValueError, match="one_hot"):
        manager.predict_volume_to_path(None)
