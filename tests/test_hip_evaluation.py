"""-m gpu: vs_confusion_matrix (csrc/evaluate.hip) bit for bit against np.bincount restatements at every size where the kernel takes
another path, the Python routes above it, and VolSeg2DPredictionManager.evaluate_volume end to end."""
import csv
import json
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from evaluation_cases import assert_scores_equal, bincount_confusion, brute_scores
from hip_helpers import DEV, lib
from volume_segmantics_amd.utilities import evaluation as ev

pytestmark = pytest.mark.gpu

GARBAGE = -0x0123456789ABCDEF


def run_kernel(truth, pred, classes, lut=None, slab_len=None):
    """the C call on flat uint8 arrays; the outputs start out full of garbage (the call must zero them)"""
    L = lib()
    t = torch.from_numpy(np.ascontiguousarray(truth).reshape(-1)).to(DEV)
    p = torch.from_numpy(np.ascontiguousarray(pred).reshape(-1)).to(DEV)
    n = t.numel()
    slab_len = n if slab_len is None else slab_len
    nslabs = -(-n // slab_len)
    lut_dev = None if lut is None else torch.from_numpy(np.asarray(lut, dtype=np.uint8)).to(DEV)
    counts = torch.full((nslabs, classes, classes), GARBAGE, dtype=torch.int64, device=DEV)
    dropped = torch.full((nslabs, 2), GARBAGE, dtype=torch.int64, device=DEV)
    L.check(L.lib.vs_confusion_matrix(L.ptr(t), L.ptr(p), n, classes, L.ptr(lut_dev), slab_len, L.ptr(counts), L.ptr(dropped), L.stream_ptr()))
    torch.cuda.synchronize()
    return counts.cpu().numpy(), dropped.cpu().numpy()


def check(truth, pred, classes, lut=None, slab_len=None):
    counts, dropped = run_kernel(truth, pred, classes, lut, slab_len)
    ref_counts, ref_dropped = bincount_confusion(truth, pred, classes, lut, slab_len)
    assert counts.shape == ref_counts.shape and dropped.shape == ref_dropped.shape
    assert np.array_equal(counts, ref_counts), (counts - ref_counts).reshape(len(counts), -1)[:4]
    assert np.array_equal(dropped, ref_dropped), (dropped, ref_dropped)
    assert counts.sum() + dropped.sum() == np.asarray(truth).size
    return counts, dropped


def uniform_labels(n, classes, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, classes, n).astype(np.uint8), rng.integers(0, classes, n).astype(np.uint8)


def test_smallest_and_one_short_slab():
    check(np.zeros(1, np.uint8), np.zeros(1, np.uint8), 1)
    check(*uniform_labels(63, 2, 0), 2)


def test_unaligned_slab_boundaries():
    t, p = uniform_labels(5 * 7 * 9, 4, 1)
    whole, _ = check(t, p, 4)
    per, _ = check(t, p, 4, slab_len=63)            # 63: every boundary splits a 16-byte vector
    assert per.shape == (5, 4, 4) and np.array_equal(per.sum(0, keepdims=True), whole)
    check(t, p, 4, slab_len=100)                    # a ragged last slab (315 = 3 * 100 + 15)


def test_aligned_slabs_per_slice():
    t, p = uniform_labels(3 * 64 * 64, 4, 2)
    per, _ = check(t, p, 4, slab_len=64 * 64)
    assert per.shape == (3, 4, 4) and (per.sum((1, 2)) == 64 * 64).all()


@pytest.mark.parametrize("classes", [5, 16])
def test_several_workgroups_and_a_ragged_tail(classes):
    n = 16 * 256 * 37 + 5
    t, p = uniform_labels(n, classes, 3 + classes)
    check(t, p, classes)
    check(t, p, classes, slab_len=70001)            # slabs longer than one item, unaligned, with a short last one


def test_constant_volume_takes_the_uniform_shortcut():
    n = 1 << 20
    counts, _ = check(np.full(n, 2, np.uint8), np.full(n, 1, np.uint8), 4)
    assert counts[0, 2, 1] == n


def test_code_change_inside_a_vector_and_inside_a_wave():
    n = 1 << 20
    t, p = np.full(n, 2, np.uint8), np.full(n, 1, np.uint8)
    t[n // 2 + 3:] = 3
    p[n // 2 + 3:] = 0
    counts, _ = check(t, p, 4)
    assert counts[0, 2, 1] == n // 2 + 3 and counts[0, 3, 0] == n - n // 2 - 3
    p[n // 4 + 17:n // 4 + 21] = 3                  # a short run inside otherwise flat lanes
    check(t, p, 4)
    check(t, p, 4, slab_len=1 << 14)


def test_large_count_needs_more_than_24_bits():
    n = (1 << 24) + 3
    counts, _ = check(np.full(n, 15, np.uint8), np.full(n, 15, np.uint8), 16)
    assert counts[0, 15, 15] == n


def lut_case():
    rng = np.random.default_rng(7)
    n = 40000 + 11
    raw = np.array([0, 7, 200, 99, 42], dtype=np.uint8)[rng.choice(5, n, p=[0.4, 0.3, 0.25, 0.03, 0.02])]   # 99: ignore, 42: unknown
    pred = rng.integers(0, 3, n).astype(np.uint8)
    lut = np.full(256, 254, dtype=np.uint8)
    lut[[0, 7, 200]] = [0, 1, 2]
    lut[99] = 255
    return raw, pred, lut


def test_lut_remap_ignore_and_invalid():
    raw, pred, lut = lut_case()
    counts, dropped = check(raw, pred, 3, lut=lut, slab_len=10000)
    assert dropped[:, 0].sum() == (raw == 99).sum() and dropped[:, 1].sum() == (raw == 42).sum() > 0
    with pytest.raises(ValueError, match=rf"{int((raw == 42).sum())} of {raw.size} voxels.*ground-truth values \[42\]"):
        ev.confusion_matrix(pred, raw, 3, label_values=[0, 7, 200], ignore_label=99, device=DEV)
    ok = raw != 42                                      # without the unknown value the wrapper returns the kernel's integers
    c, d = ev.confusion_matrix(pred[ok], raw[ok], 3, label_values=[0, 7, 200], ignore_label=99, device=DEV)
    rc, rd = bincount_confusion(raw[ok], pred[ok], 3, lut)
    assert np.array_equal(c, rc[0]) and np.array_equal(d, rd[0]) and d[0] == (raw == 99).sum()


def test_out_of_range_prediction_is_counted_not_indexed():
    t, p = uniform_labels(30000 + 7, 3, 8)
    p[::97] = 3
    p[5::1001] = 255
    counts, dropped = check(t, p, 3)
    assert dropped[0, 1] == (p >= 3).sum() and dropped[0, 0] == 0
    t[::89] = 200                                        # identity table: a truth byte >= K is invalid as well
    check(t, p, 3, slab_len=4099)
    with pytest.raises(ValueError, match="prediction values"):
        ev.confusion_matrix(p, t, 3, device=DEV)


def test_seventeen_classes_error_from_c_and_torch_route_in_python():
    L = lib()
    t, p = uniform_labels(3 * 6667, 17, 9)
    td, pd = torch.from_numpy(t).to(DEV), torch.from_numpy(p).to(DEV)
    counts = torch.zeros((1, 17, 17), dtype=torch.int64, device=DEV)
    dropped = torch.zeros((1, 2), dtype=torch.int64, device=DEV)
    rc = L.lib.vs_confusion_matrix(L.ptr(td), L.ptr(pd), t.size, 17, None, t.size, L.ptr(counts), L.ptr(dropped), L.stream_ptr())
    assert rc == -1 and "17 classes" in L.last_error()
    t3, p3 = t.reshape(3, -1), p.reshape(3, -1)
    for per_slice in (False, True):
        got = ev.confusion_matrix(p3, t3, 17, per_slice=per_slice, device=DEV)
        host = ev.confusion_matrix(p3, t3, 17, per_slice=per_slice, device="cpu")
        ref = bincount_confusion(t, p, 17, slab_len=t3.shape[1] if per_slice else None)
        for g, h, r in zip(got, host, ref):
            assert g.dtype == np.int64 and np.array_equal(g, h) and np.array_equal(g, r if per_slice else r[0])


def test_repeatable_and_python_routes_agree():
    t, p = uniform_labels(6 * 50 * 30, 4, 10)
    first, second = run_kernel(t, p, 4, slab_len=1500), run_kernel(t, p, 4, slab_len=1500)
    assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1])
    t3, p3 = t.reshape(6, 50, 30), p.reshape(6, 50, 30)
    for per_slice in (False, True):
        host = ev.confusion_matrix(p3, t3, 4, per_slice=per_slice, device="cpu")
        for pred, truth in ((p3, t3), (torch.from_numpy(p3).to(DEV), torch.from_numpy(t3).to(DEV)), (p3.astype(np.int32), t3.astype(np.int16))):
            got = ev.confusion_matrix(pred, truth, 4, per_slice=per_slice, device=DEV)
            assert np.array_equal(got[0], host[0]) and np.array_equal(got[1], host[1])
    view = torch.from_numpy(np.concatenate([np.zeros(3, np.uint8), t])).to(DEV)[3:]      # a device tensor that is not 16-byte aligned
    assert view.data_ptr() % 16 != 0
    assert np.array_equal(ev.confusion_matrix(torch.from_numpy(p).to(DEV), view, 4)[0], host[0].sum(0))


# ---- the manager -------------------------------------------------------------------------------------------------------------
TRUTH_VALUES = np.array([0, 7, 100, 200], dtype=np.uint8)
IGNORE = 255


@pytest.fixture(scope="module")
def manager_and_truth(golden, tmp_path_factory):
    from oracle.unet_resnet34_torch import seeded_oracle
    from volume_segmantics_amd.checkpoint_compat import reference_pickle_enum
    from volume_segmantics_amd.model.operations.vol_seg_prediction_manager import VolSeg2DPredictionManager
    from volume_segmantics_amd.utilities.base_data_utils import ModelType
    vol = golden("g3_predict_29x64x40_c4.npz")["vol"]
    path = tmp_path_factory.mktemp("ck") / "model.pytorch"
    torch.save({"model_state_dict": seeded_oracle(4, 0).state_dict(),
                "model_struc_dict": {"type": reference_pickle_enum(ModelType.U_NET), "encoder_name": "resnet34",
                                     "encoder_weights": "imagenet", "in_channels": 1, "classes": 4},
                "optimizer_state_dict": {}, "loss_val": 0.1, "label_codes": {"fg": 1}}, path)
    settings = SimpleNamespace(quality="low", output_probs=False, clip_data=False, st_dev_factor=2.575, data_hdf5_path="/data",
                               cuda_device=0, downsample=False, one_hot=False, prediction_axis="Z", prediction_batch_size=7,
                               evaluation_per_slice=True, evaluation_ignore_label=IGNORE)
    manager = VolSeg2DPredictionManager(str(path), vol, settings)
    rng = np.random.default_rng(11)
    classes = rng.integers(0, 4, vol.shape).astype(np.uint8)         # synthetic truth: class indices, a band to ignore, raw label values
    truth = TRUTH_VALUES[classes]
    truth[:, 10:12, :] = IGNORE
    return manager, truth, classes


@pytest.mark.parametrize("quality", ["LOW", "MEDIUM"])
def test_manager_evaluate_volume(manager_and_truth, tmp_path, quality):
    from volume_segmantics_amd.utilities import base_data_utils as utils
    manager, truth, classes = manager_and_truth
    out = tmp_path / "seg.h5"
    scores = manager.evaluate_volume(truth, out, quality=utils.Quality[quality])
    pred = manager.last_evaluation["prediction"]
    assert pred.dtype == np.uint8 and pred.shape == truth.shape
    assert np.array_equal(utils.get_numpy_from_path(out)[0], pred)                       # the label volume, written as predict does
    assert manager.last_evaluation["label_values"].tolist() == TRUTH_VALUES.tolist()     # codes {"fg": 1}: ascending unique values, no 255
    keep = truth != IGNORE
    b = brute_scores(pred[keep], classes[keep], 4)
    assert_scores_equal(scores, b)
    assert manager.last_evaluation["dropped"].tolist() == [int((~keep).sum()), 0]

    doc = json.loads((tmp_path / "seg_scores.json").read_text())
    nan_to_none = lambda xs: [None if np.isnan(x) else x for x in xs]                    # noqa: E731
    for name in ("dice", "iou", "precision", "recall"):
        assert [c[name] for c in doc["classes"]] == nan_to_none(getattr(scores, name).tolist())
    assert [c["label_value"] for c in doc["classes"]] == TRUTH_VALUES.tolist()
    assert [c["truth_voxels"] for c in doc["classes"]] == b["truth"] and [c["predicted_voxels"] for c in doc["classes"]] == b["pred"]
    assert [c["true_positives"] for c in doc["classes"]] == b["tp"]
    assert abs(doc["mean_dice"] - b["mean_dice"]) <= 1e-12 and abs(doc["mean_iou"] - b["mean_iou"]) <= 1e-12
    assert abs(doc["accuracy"] - b["accuracy"]) <= 1e-12
    assert np.array_equal(np.array(doc["confusion_matrix"]), bincount_confusion(classes[keep], pred[keep], 4)[0][0])
    assert doc["dropped"] == {"ignored": int((~keep).sum()), "invalid": 0}

    rows = list(csv.reader((tmp_path / "seg_scores.csv").open()))
    assert [r[0] for r in rows[1:]] == ["0", "1", "2", "3", "mean", "accuracy"]
    for c in range(4):
        assert [int(v) for v in rows[1 + c][1:5]] == [TRUTH_VALUES[c], b["truth"][c], b["pred"][c], b["tp"][c]]
        np.testing.assert_allclose([float(v) for v in rows[1 + c][5:9]], [b[n][c] for n in ("dice", "iou", "precision", "recall")],
                                   rtol=0, atol=1e-12, equal_nan=True)
    assert abs(float(rows[5][5]) - b["mean_dice"]) <= 1e-12 and abs(float(rows[5][6]) - b["mean_iou"]) <= 1e-12
    assert abs(float(rows[6][5]) - b["accuracy"]) <= 1e-12

    per = list(csv.reader((tmp_path / "seg_scores_per_slice.csv").open()))
    assert per[0] == ["slice", "dice_class_0", "dice_class_1", "dice_class_2", "dice_class_3"] and len(per) == 1 + truth.shape[0]
    for s in range(truth.shape[0]):
        want = brute_scores(pred[s][keep[s]], classes[s][keep[s]], 4)["dice"]
        np.testing.assert_allclose([float(v) for v in per[1 + s][1:]], want, rtol=0, atol=1e-12, equal_nan=True)

    given = manager.evaluate_volume(truth, None, prediction=pred)                        # scoring a prediction that is handed in
    assert np.array_equal(given.confusion, scores.confusion)


def test_manager_refuses_one_hot_and_shape_mismatch(manager_and_truth):
    manager, truth, _ = manager_and_truth
    with pytest.raises(ValueError, match=r"label volume has shape \(29, 64, 39\)"):
        manager.evaluate_volume(truth[:, :, :-1])
    manager.settings.one_hot = True
    try:
        with pytest.raises(ValueError, match="one_hot"):
            manager.evaluate_volume(truth)
    finally:
        manager.settings.one_hot = False
