"""-m gpu: the kernels of csrc/components.hip - vs_label_components, vs_component_sizes, vs_component_largest, vs_components_apply -
integer for integer against the oracles of tests/components_cases.py at every size where a kernel takes another path, the Python
routes above them against the host route and the committed vessels figures, and VolSeg2DPredictionManager with the postprocess
keys.  Output and workspace buffers start out full of garbage; nothing here has a tolerance."""
import functools
import json
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import components_cases as cc
from hip_helpers import DEV, lib
from volume_segmantics_amd.utilities import components as co

pytestmark = pytest.mark.gpu

GARBAGE32 = -0x01234567
GARBAGE64 = -0x0123456789ABCDEF
TZ, TY, TX = co.TILE_Z, co.TILE_Y, co.TILE_X


# ---- the kernels through the C ABI -------------------------------------------------------------------------------------------------
def run_label(vol, connectivity):
    L = lib()
    z, y, x = vol.shape
    v = torch.from_numpy(np.array(vol).reshape(-1)).to(DEV)
    comp = torch.full((v.numel(),), GARBAGE32, dtype=torch.int32, device=DEV)
    need = int(L.lib.vs_components_workspace_bytes(z, y, x))
    assert need == 4 * -(-z // TZ) * -(-y // TY) * -(-x // TX)
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device=DEV)
    L.check(L.lib.vs_label_components(L.ptr(v), z, y, x, connectivity, L.ptr(comp), L.ptr(ws), need, L.stream_ptr()))
    torch.cuda.synchronize()
    return comp.cpu().numpy().reshape(vol.shape)


def run_sizes(roots, with_touches=True):
    L = lib()
    z, y, x = roots.shape
    comp = torch.from_numpy(np.ascontiguousarray(roots).reshape(-1).astype(np.int32)).to(DEV)
    size = torch.full((comp.numel(),), GARBAGE32, dtype=torch.int32, device=DEV)
    touches = torch.full((comp.numel(),), 0xA5, dtype=torch.uint8, device=DEV) if with_touches else None
    L.check(L.lib.vs_component_sizes(L.ptr(comp), z, y, x, L.ptr(size), L.ptr(touches), L.stream_ptr()))
    torch.cuda.synchronize()
    return size.cpu().numpy(), (touches.cpu().numpy() if with_touches else None)


def run_largest(vol, size):
    L = lib()
    v = torch.from_numpy(np.array(vol).reshape(-1)).to(DEV)
    s = torch.from_numpy(size).to(DEV)
    keys = torch.full((256,), GARBAGE64, dtype=torch.int64, device=DEV)
    L.check(L.lib.vs_component_largest(L.ptr(v), L.ptr(s), v.numel(), L.ptr(keys), L.stream_ptr()))
    torch.cuda.synchronize()
    return keys.cpu().numpy()


def run_apply(vol, roots, size, touches, min_size=None, keep_root=None, hole_max=0, background=0):
    L = lib()
    dev = lambda a: torch.from_numpy(np.array(a).reshape(-1)).to(DEV)      # noqa: E731
    v, comp, s, t = dev(vol), dev(roots.astype(np.int32)), dev(size), dev(touches)
    m = np.zeros(256, dtype=np.int32)
    for value, least in (min_size or {}).items():
        m[value] = least
    k = np.full(256, -1, dtype=np.int32) if keep_root is None else np.asarray(keep_root, dtype=np.int32)
    m_dev, k_dev = dev(m), dev(k)
    out = torch.full((v.numel(),), 0xA5, dtype=torch.uint8, device=DEV)
    counts = torch.full((4,), GARBAGE64, dtype=torch.int64, device=DEV)
    L.check(L.lib.vs_components_apply(L.ptr(v), L.ptr(comp), L.ptr(s), L.ptr(t), L.ptr(m_dev), L.ptr(k_dev), background, hole_max, v.numel(),
                                      L.ptr(out), L.ptr(counts), L.stream_ptr()))
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(vol.shape), counts.cpu().tolist()


def assert_roots(vol, connectivities=cc.CONNECTIVITIES, oracle=cc.oracle_roots):
    for c in connectivities:
        got, want = run_label(vol, c), oracle(vol, c)
        assert np.array_equal(got, want), (vol.shape, c, np.argwhere(got != want)[:5])


# ---- vs_label_components -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 1), (7, 1, 5), (3, 4, 1), (1, 1, 37), (2, 3, 2), (1, 24, 40)])
def test_small_and_degenerate_shapes(shape):
    for k, density, seed in ((2, 0.5, 1), (4, 0.5, 2), (2, 0.05, 3)):
        assert_roots(cc.random_labels(shape, k, density, seed), oracle=cc.flood_roots)
    assert_roots(np.full(shape, 7, np.uint8), oracle=cc.flood_roots)


@pytest.mark.parametrize("x", [63, 64, 65, 700])
def test_rows_that_cross_lanes_waves_and_tiles(x):
    vol = cc.random_labels((2, 3, x), 2, 0.7, x)
    vol[0, 0, :] = 1                                                # one run along the whole row
    vol[1, 2, 5:x - 3] = 0
    assert_roots(vol)


@pytest.mark.parametrize("shape", [(TZ, TY, TX), (TZ + 1, TY, TX), (TZ, TY + 1, TX), (TZ, TY, TX + 1), (TZ + 1, TY + 1, TX + 1)])
def test_axes_at_and_one_beyond_the_tile(shape):
    assert_roots(cc.random_labels(shape, 2, 0.5, sum(shape)))
    assert_roots(np.zeros(shape, np.uint8), (6,))


@pytest.mark.parametrize("shape", [(5, 7, 9), (17, 33, 65), (3, 130, 70)])
@pytest.mark.parametrize("k,density", [(2, 0.5), (2, 0.05), (4, 0.5), (4, 0.05)])
def test_random_labels(shape, k, density):
    assert_roots(cc.random_labels(shape, k, density, shape[0] * 10 + k))


PLACES = [(3, 3, 30), (TZ, 3, 30), (3, TY, 30), (3, 3, TX), (TZ, TY, 30), (TZ, 3, TX), (3, TY, TX), (TZ, TY, TX), (TZ, TY - 1, TX - 1), (3, TY - 1, TX - 1)]


@pytest.mark.parametrize("kind", sorted(cc.PAIR_KINDS))
def test_two_voxels_that_touch_by_an_edge_or_a_corner(kind):
    """inside a tile, and across a tile face, edge and corner"""
    for at in PLACES:
        vol = cc.pair_touching(kind, at)
        a = int(np.flatnonzero(vol.reshape(-1))[0])
        b = int(np.flatnonzero(vol.reshape(-1))[1])
        for c in cc.CONNECTIVITIES:
            roots = run_label(vol, c).reshape(-1)
            joined = c >= cc.PAIR_KINDS[kind]
            assert roots[a] == a and roots[b] == (a if joined else b), (kind, at, c)
            assert (roots[vol.reshape(-1) == 0] == 0).all()


def test_serpentine_through_every_row():
    vol = cc.snake_rows((9, 40, 130))
    assert vol.reshape(-1)[0] == 1 and vol.reshape(-1)[-1] == 1
    for c in cc.CONNECTIVITIES:
        roots = run_label(vol, c)
        assert (roots[vol == 1] == 0).all() and roots.reshape(-1)[-1] == 0, c
        assert np.array_equal(roots, cc.oracle_roots(vol, c)), c


def test_checkerboard():
    vol = cc.checkerboard((9, 10, 70))
    n = vol.size
    assert np.array_equal(run_label(vol, 6).reshape(-1), np.arange(n))          # every voxel its own component
    assert np.array_equal(run_label(vol, 26).reshape(-1), vol.reshape(-1))     # one component per value: roots 0 and 1
    assert_roots(vol, (18,))


def test_concentric_shells_across_every_tile_boundary():
    assert_roots(cc.shells((19, 21, 135)))


def test_repeatable():
    vol = cc.random_labels((17, 33, 65), 4, 0.5, 9)
    assert np.array_equal(run_label(vol, 26), run_label(vol, 26))


# ---- vs_component_sizes, vs_component_largest, vs_components_apply -------------------------------------------------------------------
def test_sizes_of_one_solid_component():
    roots = np.zeros((40, 48, 72), dtype=np.int32)                  # every voxel adds to one root
    assert np.array_equal(run_label(np.full(roots.shape, 3, np.uint8), 6), roots)
    size, touches = run_sizes(roots)
    assert size[0] == roots.size and not size[1:].any() and touches[0] == 1 and not touches[1:].any()
    size, _ = run_sizes(roots, with_touches=False)
    assert size[0] == roots.size and not size[1:].any()


@pytest.mark.parametrize("shape,k,density", [((5, 7, 9), 4, 0.5), ((17, 33, 65), 2, 0.5), ((3, 130, 70), 4, 0.05), ((1, 24, 40), 2, 0.5), ((1, 1, 37), 2, 0.5)])
def test_sizes_and_touches_of_random_labels(shape, k, density):
    vol = cc.random_labels(shape, k, density, 5)
    roots = cc.oracle_roots(vol, 6)
    size, touches = run_sizes(roots)
    want_size, want_touches = cc.oracle_sizes(vol, roots)
    assert np.array_equal(size, want_size) and np.array_equal(touches, want_touches)


def test_touches_on_each_face_separately_and_on_a_flat_volume():
    shape = (12, 14, 70)
    for axis in range(3):
        for end in (0, shape[axis] - 1):
            vol = np.zeros(shape, np.uint8)
            vol[5, 6, 30] = 1                                       # inside: does not touch
            at = [5, 6, 40]
            at[axis] = end
            vol[tuple(at)] = 1
            roots = cc.oracle_roots(vol, 6)
            _, touches = run_sizes(roots)
            lin = np.ravel_multi_index((5, 6, 30), shape), np.ravel_multi_index(tuple(at), shape)
            assert touches[lin[0]] == 0 and touches[lin[1]] == 1 and touches[0] == 1 and touches.sum() == 2, (axis, end)
    vol = np.zeros((1, 14, 70), np.uint8)                           # z has length 1: it is no face
    vol[0, 6, 30] = 1
    _, touches = run_sizes(cc.oracle_roots(vol, 6))
    assert touches[6 * 70 + 30] == 0 and touches[0] == 1


@functools.lru_cache(maxsize=None)
def scene():
    """the cleanup scene with its oracle roots, sizes and touches under connectivity 6, once"""
    vol = cc.cleanup_scene()
    roots = cc.oracle_roots(vol, 6)
    size, touches = cc.oracle_sizes(vol, roots)
    return vol, roots, size, touches


def test_largest_with_a_tie_and_an_absent_value():
    vol, roots, size, _ = scene()
    got_size, _ = run_sizes(roots)
    assert np.array_equal(got_size, size)
    keys = run_largest(vol, size)
    want = cc.oracle_largest(vol, roots)
    for value in range(256):
        if want[value] < 0:
            assert keys[value] == 0, value                          # a value that does not occur
        else:
            assert keys[value] == (int(size[want[value]]) << 32) | (0x7FFFFFFF - int(want[value])), value
    first_twin = np.ravel_multi_index((25, 5, 5), vol.shape)
    assert want[2] == first_twin and size[first_twin] == size[np.ravel_multi_index((25, 5, 40), vol.shape)] == cc.SCENE["twin"]
    assert want[4] == -1


APPLY_CASES = {
    "nothing": dict(),
    "hole_a_at_its_size": dict(hole_max=cc.SCENE["hole_a"]),
    "hole_a_one_below": dict(hole_max=cc.SCENE["hole_a"] - 1),
    "object_3_at_its_size": dict(min_size={3: cc.SCENE["object_3"]}, hole_max=1),
    "object_3_one_above": dict(min_size={3: cc.SCENE["object_3"] + 1}, hole_max=1),       # cleared: its hole stays background
    "bar_cleared_hole_b_stays": dict(min_size={2: cc.SCENE["bar"] + 1}, hole_max=3),
    "keep_largest_of_2": dict(keep_largest={2}, hole_max=600),
    "everything": dict(min_size={1: 100, 2: 5, 3: 27}, keep_largest={1, 2}, hole_max=600),
    "background_1": dict(min_size={0: 10, 2: 28}, hole_max=100, background=1),
}


@pytest.mark.parametrize("name", sorted(APPLY_CASES))
def test_apply_against_the_oracle(name):
    vol, roots, size, touches = scene()
    case = APPLY_CASES[name]
    background = case.get("background", 0)
    keep_root = np.full(256, -1, dtype=np.int64)
    largest = cc.oracle_largest(vol, roots)
    for value in case.get("keep_largest", ()):
        keep_root[value] = largest[value]
    got, counts = run_apply(vol, roots, size, touches, case.get("min_size"), keep_root, case.get("hole_max", 0), background)
    want, totals, _ = cc.oracle_clean(vol, 6, case.get("min_size"), case.get("keep_largest"), case.get("hole_max", 0), background, roots=roots)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert counts == totals


def test_apply_fills_holes_as_the_rules_say():
    vol, roots, size, touches = scene()
    got, counts = run_apply(vol, roots, size, touches, hole_max=600)
    assert (got[8, 8, 10:15] == 1).all()                            # hole A takes the value in front of its root
    assert (got[12, 12, 24:27] == 2).all()                          # hole B borders 1 and 2: the voxel in front of its root is the bar
    assert got[33, 11, 11] == 3
    assert (got[32:34, 2:4, 71] == 0).all()                         # the pocket is open to the boundary
    assert counts == [0, 0, 3, cc.SCENE["hole_a"] + cc.SCENE["hole_b"] + cc.SCENE["hole_c"]]
    got, counts = run_apply(vol, roots, size, touches, {3: 27}, hole_max=600)
    assert (got[32:35, 10:13, 10:13] == 0).all() and counts == [1, cc.SCENE["object_3"], 2, cc.SCENE["hole_a"] + cc.SCENE["hole_b"]]


# ---- device route against host route ---------------------------------------------------------------------------------------------
ROUTE_VOLUMES = {"random": lambda: cc.random_labels((17, 33, 65), 4, 0.5, 3), "scene": cc.cleanup_scene, "shells": lambda: cc.shells((19, 21, 135)),
                 "flat": lambda: cc.random_labels((1, 24, 40), 2, 0.5, 4), "snake": lambda: cc.snake_rows((9, 40, 130))}


@pytest.mark.parametrize("name", sorted(ROUTE_VOLUMES))
def test_device_route_equals_host_route(name):
    vol = ROUTE_VOLUMES[name]()
    kw = dict(min_object_size={1: 30, 2: 5, 3: 27}, keep_largest={2: True}, fill_holes=50)
    for c in cc.CONNECTIVITIES:
        assert np.array_equal(co.label_components(vol, c, device=DEV), co.label_components(vol, c, device="cpu")), c
        assert co.component_table(vol, c, device=DEV) == co.component_table(vol, c, device="cpu"), c
        got, report = co.clean_label_volume(vol, connectivity=c, device=DEV, **kw)
        want, want_report = co.clean_label_volume(vol, connectivity=c, device="cpu", **kw)
        assert got.dtype == np.uint8 and np.array_equal(got, want) and report == want_report, c
        oracle, totals, rows = cc.oracle_clean(vol, c, {1: 30, 2: 5, 3: 27}, {2}, 50)
        assert np.array_equal(got, oracle) and report["values"] == rows and [report["holes_filled"], report["voxels_filled"]] == totals[2:]


def test_device_route_takes_tensors_wide_dtypes_and_unaligned_views():
    vol = cc.cleanup_scene()
    want = co.label_components(vol, 18, device="cpu")
    dev = torch.from_numpy(np.array(vol)).to(DEV)
    assert np.array_equal(co.label_components(dev, 18), want)       # a device tensor chooses the device
    assert np.array_equal(co.label_components(vol.astype(np.int32), 18, device=DEV), want)
    assert np.array_equal(co.label_components(dev.to(torch.int64), 18), want)
    view = torch.from_numpy(np.concatenate([np.zeros(3, np.uint8), vol.reshape(-1)])).to(DEV)[3:].reshape(vol.shape)
    assert view.data_ptr() % 16 != 0
    assert np.array_equal(co.label_components(view, 18), want)
    got, _ = co.clean_label_volume(view, min_object_size=27, fill_holes=10)
    assert np.array_equal(got, co.clean_label_volume(vol, min_object_size=27, fill_holes=10, device="cpu")[0])
    with pytest.raises(ValueError, match="do not fit uint8"):
        co.label_components(dev.to(torch.int32) + 300, device=DEV)


@functools.lru_cache(maxsize=None)
def vessels_host(connectivity):
    """roots, cleaned volume and report of the host route on the vessels fixture, once"""
    vol = cc.vessels()
    roots = co.label_components(vol, connectivity, device="cpu")
    min_size = co._per_value(80000, int, 0, "min_object_size")
    settings = dict(connectivity=connectivity, background=0, fill_holes=600, min_object_size={str(c): 80000 for c in range(1, 256)}, keep_largest=[])
    cleaned, report = co._clean_host(vol, roots, min_size, np.zeros(256, dtype=bool), 600, 0, settings)
    return roots, cleaned, report


def test_vessels_fixture_all_three_connectivities():
    vol = cc.vessels()
    expected = cc.vessels_expected()["connectivity"]
    dev = torch.from_numpy(np.array(vol)).to(DEV)
    for c in cc.CONNECTIVITIES:
        roots, cleaned, report = vessels_host(c)
        got_roots = co.label_components(dev, c)
        assert np.array_equal(got_roots, roots), c
        assert np.array_equal(co.label_components(dev, c), got_roots), c                    # the same bits on a second call
        table = co.component_table(dev, c)
        assert {str(k): v for k, v in table.items()} == expected[str(c)]["table"], c
        got, got_report = co.clean_label_volume(dev, min_object_size=80000, fill_holes=600, connectivity=c)
        assert np.array_equal(got, cleaned) and got_report == report, c
        for name, kw in cc.VESSELS_CLEANUPS.items():
            out, rep = co.clean_label_volume(dev, connectivity=c, **kw)
            want = expected[str(c)]["cleanups"][name]
            assert rep["values"] == want["values"] and [rep["holes_filled"], rep["voxels_filled"]] == [want["holes_filled"], want["voxels_filled"]], (c, name)
            assert {str(int(k)): int(n) for k, n in zip(*np.unique(out, return_counts=True))} == want["voxels_of_value"], (c, name)


# ---- error paths -----------------------------------------------------------------------------------------------------------------
def test_errors_are_reported_and_the_next_call_works():
    L = lib()
    shape = (9, 9, 65)
    n = int(np.prod(shape))
    v = torch.zeros(n, dtype=torch.uint8, device=DEV)
    comp = torch.zeros(n, dtype=torch.int32, device=DEV)
    need = int(L.lib.vs_components_workspace_bytes(*shape))
    assert need == 4 * 2 * 2 * 2
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    rc = L.lib.vs_label_components(L.ptr(v), *shape, 6, L.ptr(comp), L.ptr(ws), need - 1, L.stream_ptr())
    assert rc == -1 and "workspace" in L.last_error() and str(need) in L.last_error()
    rc = L.lib.vs_label_components(L.ptr(v), *shape, 6, None, L.ptr(ws), need, L.stream_ptr())
    assert rc == -1 and "null" in L.last_error()
    rc = L.lib.vs_label_components(L.ptr(v), *shape, 7, L.ptr(comp), L.ptr(ws), need, L.stream_ptr())
    assert rc == -1 and "connectivity 7" in L.last_error()
    for extents in ((1 << 31, 1, 1), (2048, 1024, 1024), (1, 46341, 46341), (0, 4, 4)):
        assert L.lib.vs_components_workspace_bytes(*extents) == 0
        rc = L.lib.vs_label_components(L.ptr(v), *extents, 6, L.ptr(comp), L.ptr(ws), need, L.stream_ptr())       # nothing is touched
        assert rc == -1 and "2^31" in L.last_error(), extents
        rc = L.lib.vs_component_sizes(L.ptr(comp), *extents, L.ptr(comp), None, L.stream_ptr())
        assert rc == -1 and "2^31" in L.last_error(), extents
    rc = L.lib.vs_component_sizes(L.ptr(comp), *shape, None, None, L.stream_ptr())
    assert rc == -1 and "null" in L.last_error()
    rc = L.lib.vs_component_largest(L.ptr(v), L.ptr(comp), 1 << 31, L.ptr(comp), L.stream_ptr())
    assert rc == -1 and "2^31" in L.last_error()
    rc = L.lib.vs_components_apply(L.ptr(v), L.ptr(comp), L.ptr(comp), None, L.ptr(comp), L.ptr(comp), 0, 5, n, L.ptr(v), L.ptr(comp), L.stream_ptr())
    assert rc == -1 and "touches" in L.last_error()
    rc = L.lib.vs_components_apply(L.ptr(v), L.ptr(comp), L.ptr(comp), None, L.ptr(comp), L.ptr(comp), 0, 0, n, L.ptr(v), L.ptr(comp), L.stream_ptr())
    assert rc == -1 and "overlap" in L.last_error()
    with pytest.raises(ValueError, match="connectivity 7"):
        co.label_components(v.reshape(shape), 7)
    with pytest.raises(ValueError, match="2\\^31"):
        co.label_components(torch.zeros(1, device=DEV, dtype=torch.uint8).expand(2048, 1024, 1024))               # a view: no memory behind it
    vol = cc.random_labels((5, 7, 9), 4, 0.5, 8)
    assert_roots(vol, oracle=cc.flood_roots)


def test_too_little_device_memory_is_a_value_error(monkeypatch):
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda device=None: (1000, 1 << 30))
    with pytest.raises(ValueError, match=r"needs \d+ bytes of device memory but only 1000 bytes are free"):
        co.clean_label_volume(cc.cleanup_scene(), min_object_size=5, device=DEV)
    with pytest.raises(ValueError, match=r"needs \d+ bytes of device memory but only 1000 bytes are free"):
        co.label_components(cc.cleanup_scene(), device=DEV)


# ---- the manager -------------------------------------------------------------------------------------------------------------------
def test_manager_cleans_the_merged_volume(golden, tmp_path):
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
    settings = SimpleNamespace(quality="low", output_probs=True, clip_data=False, st_dev_factor=2.575, data_hdf5_path="/data",
                               cuda_device=0, downsample=False, one_hot=False, prediction_axis="Z", prediction_batch_size=7)
    manager = VolSeg2DPredictionManager(str(path), vol, settings)
    for name in ("absent", "off", "on"):
        (tmp_path / name).mkdir()

    raw = manager.predict_volume_to_path(tmp_path / "absent" / "seg.npy")
    assert getattr(manager, "last_postprocess", None) is None
    settings.postprocess_min_object_size = 0                        # present but inactive: nothing runs
    settings.postprocess_keep_largest = False
    settings.postprocess_fill_holes = 0
    same = manager.predict_volume_to_path(tmp_path / "off" / "seg.npy")
    assert np.array_equal(same, raw) and getattr(manager, "last_postprocess", None) is None
    assert (tmp_path / "off" / "seg.npy").read_bytes() == (tmp_path / "absent" / "seg.npy").read_bytes()
    assert sorted(p.name for p in (tmp_path / "off").iterdir()) == sorted(p.name for p in (tmp_path / "absent").iterdir()) == ["seg.npy", "seg_probs.h5"]

    settings.postprocess_min_object_size = 6
    settings.postprocess_fill_holes = 4
    settings.postprocess_connectivity = 26
    cleaned = manager.predict_volume_to_path(tmp_path / "on" / "seg.npy")
    assert np.array_equal(manager.last_postprocess["raw"], raw)
    want, totals, rows = cc.oracle_clean(raw, 26, {c: 6 for c in range(1, 256)}, None, 4)
    assert totals[0] > 0 and np.array_equal(cleaned, want) and np.array_equal(np.load(tmp_path / "on" / "seg.npy"), want)
    report = manager.last_postprocess["report"]
    assert report["values"] == rows and [report["holes_filled"], report["voxels_filled"]] == totals[2:] and report["connectivity"] == 26
    assert json.loads((tmp_path / "on" / "seg_components.json").read_text()) == report
    assert (tmp_path / "on" / "seg_components.csv").is_file()
    from volume_segmantics_amd.utilities.base_data_utils import numpy_from_hdf5
    probs = [numpy_from_hdf5(tmp_path / name / "seg_probs.h5")[0] for name in ("absent", "on")]
    assert probs[0].dtype == probs[1].dtype and np.array_equal(probs[0], probs[1])

    settings.one_hot = True
    with pytest.raises(ValueError, match="one_hot"):
        manager.predict_volume_to_path(None)
