"""-m gpu: vs_thickness_centres, vs_thickness_paint and vs_thickness_resolve (csrc/thickness.hip) through the C ABI behind vs_edt_squared,
integer for integer against the brute-force oracle of tests/thickness_cases.py - the centre list as a set, the levels of the sparse
table after the resolve, T2 - on the named volumes and at every size where the kernels take another path: rows that end before, on
and after a 64-lane boundary, Y and Z of 1, spans on every level, a list painted in several calls; then determinism, the Python
route on the device against the host route, the work bound, the refusals, the whole vessels fixture, the command and
VolSeg2DPredictionManager with the thickness keys.  Buffers start out full of garbage; nothing here has a tolerance."""
import json
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import components_cases as cc
import thickness_cases as tc
from hip_helpers import DEV, lib
from volume_segmantics_amd.utilities import label_volume as lv
from volume_segmantics_amd.utilities import thickness as th

pytestmark = pytest.mark.gpu

GARBAGE32 = -0x01234567
GARBAGE64 = -0x0123456789ABCDEF


# ---- the kernels through the C ABI -------------------------------------------------------------------------------------------------
def run_r(vol, value):
    """R on the device: vs_edt_squared with the seeds labels != value (int32 tensor holding uint32 bits)"""
    L = lib()
    shape = tuple(vol.shape)
    seeds = torch.from_numpy((np.asarray(vol) != value).astype(np.uint8).reshape(-1)).to(DEV)
    r = torch.full((seeds.numel(),), GARBAGE32, dtype=torch.int32, device=DEV)
    need = L.lib.vs_edt_workspace_bytes(*shape)
    work = torch.empty(need, dtype=torch.uint8, device=DEV)
    L.check(L.lib.vs_edt_squared(L.ptr(seeds), *shape, L.ptr(r), L.ptr(work) if need else None, need, L.stream_ptr()))
    return r


def run_centres(r, shape, need):
    """(the centre list as it came, [centres, row spans]); one slot of garbage behind the list must stay"""
    L = lib()
    capacity = int((r != 0).sum())
    centres = torch.full((capacity + 1,), GARBAGE32, dtype=torch.int32, device=DEV)
    totals = torch.full((2,), GARBAGE64, dtype=torch.int64, device=DEV)
    table = None if need is None else torch.from_numpy(np.ascontiguousarray(need).view(np.int32)).to(DEV)
    L.check(L.lib.vs_thickness_centres(L.ptr(r), *shape, L.ptr(table), 0 if need is None else need.shape[1], L.ptr(centres), capacity, L.ptr(totals),
                                       L.stream_ptr()))
    torch.cuda.synchronize()
    count, rows = totals.cpu().tolist()
    assert 0 <= count <= capacity and int(centres[-1]) == GARBAGE32
    return centres[:count].clone(), [count, rows]


def run_paint_resolve(labels, r, shape, value, centres, max_r, pieces=1, t2=None):
    """(the K levels after the resolve, T2); the centre list goes in `pieces` calls"""
    L = lib()
    n = r.numel()
    need = L.lib.vs_thickness_workspace_bytes(*shape, max_r)
    levels = th.table_levels(shape[2], max_r)
    assert need == 4 * levels * n
    work = torch.full((need + 16,), 0xA5, dtype=torch.uint8, device=DEV)
    count = centres.numel()
    cuts = [count * i // pieces for i in range(pieces + 1)]
    for i in range(pieces):
        L.check(L.lib.vs_thickness_paint(L.ptr(r), *shape, centres.data_ptr() + 4 * cuts[i], cuts[i + 1] - cuts[i], max_r, max_r, L.ptr(work), need,
                                         int(i == 0), L.stream_ptr()))
    if t2 is None:
        t2 = torch.full((n,), GARBAGE32, dtype=torch.int32, device=DEV)
    L.check(L.lib.vs_thickness_resolve(L.ptr(labels), *shape, value, max_r, L.ptr(work), need, L.ptr(t2), L.stream_ptr()))
    torch.cuda.synchronize()
    assert (work[need:] == 0xA5).all()                                   # nothing behind the table is touched
    return work[:need].view(torch.int32).reshape(levels, n).cpu().numpy().view(np.uint32), t2


def assert_thickness(vol, value, want=None, pieces=1):
    """the three kernels against the oracle (and, level for level, against the host's table of the same centres)"""
    vol = np.asarray(vol)
    shape = tuple(vol.shape)
    r_want = tc.exact_r(vol, value).astype(np.uint32)
    want = tc.oracle_t2(vol, value) if want is None else want
    labels = torch.from_numpy(vol.reshape(-1).copy()).to(DEV)
    r = run_r(vol, value)
    assert np.array_equal(r.cpu().numpy().view(np.uint32).reshape(shape), r_want)
    max_r = int(r_want.max())
    every, totals = run_centres(r, shape, None)
    assert np.array_equal(np.sort(every.cpu().numpy()), tc.oracle_centres_all(vol, value))
    need = th.need_table(max_r)
    centres, totals = run_centres(r, shape, need)
    kept = th.centres_host(r_want, need)
    assert np.array_equal(np.sort(centres.cpu().numpy()), kept)
    z, y, _ = np.unravel_index(kept, shape)
    assert totals == [len(kept), int(th._ball_rows(z.astype(np.int64), y.astype(np.int64), r_want.reshape(-1)[kept], shape).sum())]
    levels, t2 = run_paint_resolve(labels, r, shape, value, centres, max_r, pieces)
    assert np.array_equal(levels[0].reshape(shape), want)               # the balls lie inside the value: the painted map IS T2
    assert np.array_equal(levels, th.resolve_host(th.paint_host(r_want, kept, len(levels)), shape[2]))
    got = t2.cpu().numpy()
    member = vol.reshape(-1) == value
    assert np.array_equal(got.view(np.uint32)[member], want.reshape(-1)[member]) and (got[~member] == GARBAGE32).all()
    levels_all, _ = run_paint_resolve(labels, r, shape, value, every, max_r, pieces)         # dropping nothing paints the same map
    assert np.array_equal(levels_all[0], levels[0])


@pytest.mark.parametrize("name", sorted(set(tc.VOLUMES) - {"filled"}))
def test_named_volumes_against_the_oracle(name):
    vol = tc.VOLUMES[name]()
    for value in tc.values_of(vol):
        assert_thickness(vol, value, tc.oracle_cached(name, value))


@pytest.mark.parametrize("x", [62, 63, 64, 65, 127, 128, 129])
def test_rows_that_end_before_on_and_after_a_wave(x):
    """a thick slab over whole rows and a bar that stops short: spans of every length up to the row's, clipped at both ends"""
    assert_thickness(tc.slab(x), 1)


@pytest.mark.parametrize("shape", [(1, 1, 130), (7, 1, 70), (1, 9, 66)])
def test_axes_of_length_one(shape):
    vol = (tc._smooth_field(shape, 7) > 0.45).astype(np.uint8)
    vol[..., -1] = 1
    vol[..., 5] = 0
    assert_thickness(vol, 1)


def test_a_list_painted_in_several_calls():
    assert_thickness(tc.blobs(), 1, tc.oracle_cached("blobs", 1), pieces=5)
    assert_thickness(tc.disc_prism(), 1, tc.oracle_cached("disc_prism", 1), pieces=3)


def test_value_without_another_value_has_no_centres():
    vol = tc.filled()
    r = run_r(vol, 3)
    assert (r == -1).all()                                               # 0xFFFFFFFF
    centres, totals = run_centres(torch.full_like(r, -1), vol.shape, None)
    assert totals == [0, 0] and centres.numel() == 0
    assert not th.local_thickness_squared(vol, 3, device=DEV).any()


def test_two_calls_give_equal_bytes():
    vol = tc.vessels_crop()
    labels = torch.from_numpy(vol.reshape(-1).copy()).to(DEV)
    r = run_r(vol, 255)
    max_r = int(r.max())
    runs = []
    for _ in range(2):
        centres, totals = run_centres(r, vol.shape, th.need_table(max_r))
        levels, t2 = run_paint_resolve(labels, r, vol.shape, 255, centres, max_r)
        runs.append((np.sort(centres.cpu().numpy()).tobytes(), totals, levels.tobytes(), t2.cpu().numpy().tobytes()))
    assert runs[0] == runs[1]


def test_errors():
    L = lib()
    vol = tc.blobs()
    shape = vol.shape
    labels = torch.from_numpy(vol.reshape(-1).copy()).to(DEV)
    r = run_r(vol, 1)
    max_r = int(r.max())
    centres, _ = run_centres(r, shape, None)
    need = L.lib.vs_thickness_workspace_bytes(*shape, max_r)
    work = torch.zeros(need, dtype=torch.uint8, device=DEV)
    out = torch.zeros(r.numel(), dtype=torch.int64, device=DEV)
    P, S = L.ptr, L.stream_ptr()
    for extents in ((2048, 1024, 1024), (1 << 31, 1, 1), (0, 4, 4), (1, 2, 70000)):
        assert L.lib.vs_thickness_workspace_bytes(*extents, 5) == 0
        assert L.lib.vs_thickness_centres(P(r), *extents, None, 0, P(out), 4, P(out), S) == -1 and "2^31" in L.last_error(), extents
        assert L.lib.vs_thickness_paint(P(r), *extents, P(centres), 1, 5, 5, P(work), need, 1, S) == -1 and "2^31" in L.last_error(), extents
        assert L.lib.vs_thickness_resolve(P(labels), *extents, 1, 5, P(work), need, P(out), S) == -1 and "2^31" in L.last_error(), extents
    for bad_r in (0, -3, 0xFFFFFFFF):
        assert L.lib.vs_thickness_workspace_bytes(*shape, bad_r) == 0
        assert L.lib.vs_thickness_paint(P(r), *shape, P(centres), 1, 1, bad_r, P(work), need, 1, S) == -1 and "squared radi" in L.last_error()
        assert L.lib.vs_thickness_resolve(P(labels), *shape, 1, bad_r, P(work), need, P(out), S) == -1 and "squared radius" in L.last_error()
    assert L.lib.vs_thickness_paint(P(r), *shape, P(centres), 1, max_r + 1, max_r, P(work), need, 1, S) == -1 and "largest" in L.last_error()
    assert L.lib.vs_thickness_paint(P(r), *shape, P(centres), r.numel() + 1, 1, max_r, P(work), need, 1, S) == -1 and "centres" in L.last_error()
    assert L.lib.vs_thickness_paint(P(r), *shape, P(centres), 1, 1, max_r, P(work), need - 4, 1, S) == -1 and "workspace" in L.last_error()
    assert L.lib.vs_thickness_paint(P(r), *shape, P(centres), 1, 1, max_r, None, need, 1, S) == -1 and "null" in L.last_error()
    assert L.lib.vs_thickness_resolve(P(labels), *shape, 256, max_r, P(work), need, P(out), S) == -1 and "uint8" in L.last_error()
    assert L.lib.vs_thickness_resolve(P(labels), *shape, 1, max_r, P(work), need - 4, P(out), S) == -1 and "workspace" in L.last_error()
    assert L.lib.vs_thickness_resolve(P(labels), *shape, 1, max_r, P(work), need, None, S) == -1 and "null" in L.last_error()
    assert L.lib.vs_thickness_centres(None, *shape, None, 0, P(out), 4, P(out), S) == -1 and "null" in L.last_error()
    assert L.lib.vs_thickness_centres(P(r), *shape, None, 7, P(out), 4, P(out), S) == -1 and "table" in L.last_error()
    assert L.lib.vs_thickness_centres(P(r), *shape, None, 0, P(out), -1, P(out), S) == -1 and "capacity" in L.last_error()
    # a list cut short by its capacity is reported, not overrun; entries outside the volume are skipped
    few = torch.full((5,), GARBAGE32, dtype=torch.int32, device=DEV)
    totals = torch.zeros(2, dtype=torch.int64, device=DEV)
    L.check(L.lib.vs_thickness_centres(P(r), *shape, None, 0, P(few), 4, P(totals), S))
    assert int(totals[0]) == int((vol == 1).sum()) and int(few[4]) == GARBAGE32 and (few[:4] >= 0).all()
    wild = torch.cat([centres, torch.tensor([-5, r.numel(), 2 ** 31 - 1], dtype=torch.int32, device=DEV)])
    levels, _ = run_paint_resolve(labels, r, shape, 1, wild, max_r)
    assert np.array_equal(levels[0].reshape(shape), tc.oracle_cached("blobs", 1))       # and the next call works


# ---- the Python route --------------------------------------------------------------------------------------------------------------
ROUTE_VOLUMES = {"crop": tc.vessels_crop, "touching": tc.touching, "flat": lambda: tc.blobs((1, 30, 34), 2), "debris": tc.debris,
                 "random": lambda: cc.random_labels((17, 33, 65), 4, 0.8, 3)}


@pytest.mark.parametrize("name", sorted(ROUTE_VOLUMES))
def test_device_route_equals_host_route(name):
    vol = ROUTE_VOLUMES[name]()
    values = sorted(np.unique(vol).tolist())[int(name == "crop"):]         # the crop without its background: a host route of seconds
    settings = SimpleNamespace(thickness_values=values, thickness_voxel_size=0.7, thickness_save_volume=True)
    got, want = th.thickness_label_volume(vol, settings, device=DEV), th.thickness_label_volume(vol, settings, device="cpu")
    assert got["squared"].dtype == np.uint32 and np.array_equal(got["squared"], want["squared"]) and np.array_equal(got["volume"], want["volume"])
    assert list(got["values"]) == list(want["values"]) and got["shape"] == want["shape"]
    for value in got["values"]:
        a, b = got["values"][value], want["values"][value]
        assert np.array_equal(a["histogram"], b["histogram"]) and json.dumps(a["figures"]) == json.dumps(b["figures"])      # bit for bit
        assert [a[k] for k in ("max_squared_radius", "centres", "row_spans", "levels", "workspace_bytes")] == \
               [b[k] for k in ("max_squared_radius", "centres", "row_spans", "levels", "workspace_bytes")]
    dev = torch.from_numpy(np.array(vol)).to(DEV)                         # a device tensor chooses the device
    assert np.array_equal(th.thickness_label_volume(dev, settings)["squared"], want["squared"])
    value = int(vol.max())
    assert np.array_equal(th.thickness_histogram(got["squared"], vol, value, device=DEV), want["values"][value]["histogram"])


def test_several_values_share_one_map():
    vol = tc.touching()
    t = th.thickness_label_volume(vol, SimpleNamespace(thickness_values=[0, 1, 2]), device=DEV)
    want = sum(tc.oracle_t2(vol, value).astype(np.int64) for value in (0, 1, 2))
    assert np.array_equal(t["squared"], want)
    assert np.array_equal(th.local_thickness_squared(vol, 2, device=DEV), tc.oracle_cached("touching", 2))


def test_several_launches_of_bounded_work(monkeypatch):
    vol = tc.vessels_crop()
    monkeypatch.setattr(th, "LAUNCH_ROWS", 1 << 14)
    t2 = torch.zeros(vol.size, dtype=torch.int32, device=DEV)
    info = th._value_device(lv.aligned_u8(vol, torch.device(DEV)), vol.shape, 255, t2, None)
    assert info["launches"] > 3
    assert np.array_equal(t2.cpu().numpy().view(np.uint32).reshape(vol.shape), tc.oracle_cached("vessels_crop", 255))


def test_work_bound_raises_without_a_launch(monkeypatch):
    vol = tc.blobs()
    rows = th.thickness_label_volume(vol, SimpleNamespace(), device="cpu")["values"][1]["row_spans"]
    L = lib()
    monkeypatch.setattr(L.lib, "vs_thickness_paint", lambda *a: pytest.fail("painted past the work bound"))
    monkeypatch.setattr(L.lib, "vs_thickness_resolve", lambda *a: pytest.fail("resolved past the work bound"))
    with pytest.raises(ValueError, match=f"paints {rows} row spans, more than thickness_max_work = {rows - 1}"):
        th.local_thickness_squared(vol, 1, device=DEV, max_work=rows - 1)
    with pytest.raises(ValueError, match="thickness_max_work = 3"):
        th.thickness_label_volume(vol, SimpleNamespace(thickness_max_work=3), device=DEV)


def test_too_little_device_memory_is_a_value_error(monkeypatch):
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda device=None: (1000, 1 << 30))
    with pytest.raises(ValueError, match=r"needs \d+ bytes of device memory but only 1000 bytes are free"):
        th.local_thickness_squared(tc.blobs(), 1, device=DEV)


def test_device_route_takes_unaligned_views_and_wide_labels():
    vol = tc.blobs()
    want = tc.oracle_cached("blobs", 1)
    dev = torch.from_numpy(np.array(vol)).to(DEV)
    assert np.array_equal(th.local_thickness_squared(dev.to(torch.int64), 1), want)
    view = torch.from_numpy(np.concatenate([np.zeros(3, np.uint8), vol.reshape(-1)])).to(DEV)[3:].reshape(vol.shape)
    assert view.data_ptr() % 16 != 0
    assert np.array_equal(th.local_thickness_squared(view, 1), want)
    with pytest.raises(ValueError, match="uint8"):
        th.local_thickness_squared(dev, 300)


# ---- the vessels fixture -------------------------------------------------------------------------------------------------------------
def test_whole_vessels_volume_once():
    """256^3, 5.9 million vessel voxels, through the internal call that keeps R: T2 >= R on M, T2 <= max R, T2 = 0 off M, and the voxels
    deep inside the crop of tests/golden/thickness_vessels.json equal the crop's own T2.  Deep is further than 2 sqrt(max R of the
    crop) from the crop's faces: a ball that contains such a voxel u has its centre v within sqrt(max R) of u (a larger ball from
    outside the crop would leave a voxel of the crop with R above the crop's maximum), and the nearest other voxel of v within
    sqrt(max R) of v - both inside the crop, so the crop sees the same R(v).  At sqrt(max R) alone the second step fails, and on this
    volume one voxel does differ there."""
    vol = cc.vessels()
    v = lv.aligned_u8(vol, torch.device(DEV))
    t2 = torch.zeros(v.numel(), dtype=torch.int32, device=DEV)
    info = th._value_device(v, vol.shape, 255, t2, th.DEFAULT_MAX_WORK, keep_table=True)
    member = v == 255
    r = info["r"]
    assert info["voxels"] == int(member.sum()) == 5879454 and 0 < info["centres"] < info["voxels"] // 2
    assert bool((t2[member] >= r[member]).all()) and int(t2.max()) == info["max_r"] == int(r.max()) and not bool(t2[~member].any())
    assert int(info["table"][0].ne(t2).sum()) == 0
    hist = th._histogram_device(v, 255, t2, vol.shape)
    assert hist.sum() == info["voxels"] and hist[0] == 0 and len(hist) == info["max_r"] + 1
    (z, y, x), (dz, dy, dx) = tc.CROP["offset"], tc.CROP["shape"]
    crop = tc.oracle_cached("vessels_crop", 255)
    k = int(math.floor(2.0 * math.sqrt(tc.vessels_expected()["max_squared_radius"]))) + 1
    inner = t2.cpu().numpy().view(np.uint32).reshape(vol.shape)[z + k:z + dz - k, y + k:y + dy - k, x + k:x + dx - k]
    assert inner.size > 0 and inner.any() and np.array_equal(inner, crop[k:dz - k, k:dy - k, k:dx - k])


def test_thickness_command_on_the_vessels_crop(tmp_path):
    from volume_segmantics_amd.scripts import thickness_2d_prediction
    from volume_segmantics_amd.utilities import base_data_utils as utils
    utils.save_data_to_hdf5(tc.vessels_crop(), tmp_path / "crop.h5")
    thickness_2d_prediction.main([str(tmp_path / "crop.h5"), "--data_dir", str(tmp_path), "--output", str(tmp_path / "vessels")])
    doc, want = json.loads((tmp_path / "vessels_thickness.json").read_text()), tc.vessels_expected()
    assert doc["values"]["255"]["histogram"] == want["histogram"] and doc["values"]["255"]["max_squared_radius"] == want["max_squared_radius"]
    for name in th.FIGURES:
        assert doc["values"]["255"][name] == pytest.approx(want["figures"][name], rel=1e-12, abs=0.0)


# ---- the manager -------------------------------------------------------------------------------------------------------------------
def test_manager_measures_the_saved_volume(golden, tmp_path):
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
    for name in ("absent", "on"):
        (tmp_path / name).mkdir()
    raw = manager.predict_volume_to_path(tmp_path / "absent" / "seg.npy")
    assert manager.last_thickness is None and [p.name for p in (tmp_path / "absent").iterdir()] == ["seg.npy"]

    settings.thickness_map, settings.thickness_voxel_size, settings.thickness_save_volume = True, 2.0, True
    same = manager.predict_volume_to_path(tmp_path / "on" / "seg.npy")
    assert np.array_equal(same, raw) and (tmp_path / "on" / "seg.npy").read_bytes() == (tmp_path / "absent" / "seg.npy").read_bytes()
    values = [v for v in np.unique(raw).tolist() if v != 0]
    assert len(values) >= 1
    assert sorted(p.name for p in (tmp_path / "on").iterdir()) == ["seg.npy", "seg_thickness.csv", "seg_thickness.h5", "seg_thickness.json"]
    want = th.thickness_label_volume(raw, settings, device="cpu")
    kept = manager.last_thickness
    assert np.array_equal(kept["squared"], want["squared"]) and list(kept["values"]) == values
    doc = json.loads((tmp_path / "on" / "seg_thickness.json").read_text())
    assert list(doc["values"]) == [str(v) for v in values] and doc["settings"]["voxel_size"] == 2.0
    for value in values:
        assert json.dumps(kept["values"][value]["figures"]) == json.dumps(want["values"][value]["figures"])
        assert doc["values"][str(value)]["voxels"] == int((raw == value).sum())

    settings.one_hot = True
    with pytest.raises(ValueError, match="one_hot"):
        manager.predict_volume_to_path(None)
