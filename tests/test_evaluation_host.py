"""Scoring a label volume against ground truth, the host side (utilities/evaluation.py, the evaluate command): the scores against a
brute-force restatement with boolean masks, the absent-class convention, the label-value rule, the NumPy counting route and the
command on existing label volumes.  The HIP kernel itself: tests/test_hip_evaluation.py."""
import csv
import ctypes
import json
import re
from pathlib import Path

import numpy as np
import pytest

from evaluation_cases import assert_scores_equal, brute_scores, random_pair
from volume_segmantics_amd.utilities import evaluation as ev

REPO = Path(__file__).resolve().parent.parent


# ---- C ABI -------------------------------------------------------------------------------------------------------------------
def test_confusion_matrix_is_declared_exported_and_bound():
    from volume_segmantics_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "volseg_hip.h").read_text(), flags=re.S)
    assert re.search(r"\bint\s+vs_confusion_matrix\s*\(", header)
    assert hasattr(ctypes.CDLL(str(_lib.LIB_PATH)), "vs_confusion_matrix")
    res, args = _lib._SIGS["vs_confusion_matrix"]
    assert res is ctypes.c_int and len(args) == 9 and args[2] is ctypes.c_int64 and args[5] is ctypes.c_int64
    assert _lib.lib.vs_confusion_matrix.argtypes == args


# ---- scores ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("classes", [2, 4, 7])
def test_scores_equal_the_boolean_mask_restatement(classes):
    pred, truth = random_pair(classes, seed=classes)
    counts, dropped = ev.confusion_matrix(pred, truth, classes, device="cpu")
    assert counts.dtype == np.int64 and counts.shape == (classes, classes) and dropped.tolist() == [0, 0]
    assert counts.sum() == pred.size
    assert_scores_equal(ev.scores_from_confusion(counts), brute_scores(pred, truth, classes))


def test_class_absent_from_both_is_nan_and_left_out_of_the_means():
    pred, truth = random_pair(3, seed=1)          # classes 0..2 occur; class 3 of 4 never does
    s = ev.scores_from_confusion(ev.confusion_matrix(pred, truth, 4, device="cpu")[0])
    assert all(np.isnan(getattr(s, n)[3]) for n in ("dice", "iou", "precision", "recall"))
    assert not np.isnan(s.dice[:3]).any()
    assert abs(s.mean_dice - s.dice[:3].mean()) <= 1e-12 and abs(s.mean_iou - s.iou[:3].mean()) <= 1e-12
    assert_scores_equal(s, brute_scores(pred, truth, 4))


def test_class_absent_from_truth_but_predicted_scores_zero_and_stays_in_the_means():
    pred, truth = random_pair(3, seed=2)
    pred = pred.copy()
    pred[0, 0, :5] = 3                             # predicted, never true
    s = ev.scores_from_confusion(ev.confusion_matrix(pred, truth, 4, device="cpu")[0])
    assert s.dice[3] == 0.0 and s.iou[3] == 0.0 and s.precision[3] == 0.0 and np.isnan(s.recall[3])
    assert abs(s.mean_dice - s.dice.mean()) <= 1e-12 and abs(s.mean_iou - s.iou.mean()) <= 1e-12
    assert_scores_equal(s, brute_scores(pred, truth, 4))


@pytest.mark.parametrize("classes", [2, 4])
def test_mean_iou_equals_the_trainers_metric_when_every_class_is_present(classes):
    """data.losses.MeanIoU (pinned to the reference by golden g6) on the one-hot of the same hard labels, one sample, CPU tensors;
    1e-6 relative = float32 arithmetic over a handful of operations."""
    import torch
    from volume_segmantics_amd.data.losses import MeanIoU
    pred, truth = random_pair(classes, shape=(1, 37, 41), seed=10 + classes)
    assert all((truth == c).any() and (pred == c).any() for c in range(classes))
    onehot = lambda a: torch.nn.functional.one_hot(torch.from_numpy(a.astype(np.int64)), classes).permute(0, 3, 1, 2)   # noqa: E731
    metric = float(MeanIoU()(onehot(pred).float(), onehot(truth).to(torch.uint8)))
    s = ev.scores_from_confusion(ev.confusion_matrix(pred, truth, classes, device="cpu")[0])
    assert abs(s.mean_iou - metric) <= 1e-6 * abs(metric), (s.mean_iou, metric)


# ---- the mapping rule ----------------------------------------------------------------------------------------------------------
def test_truth_label_values():
    truth = np.array([0, 7, 200, 7, 0], dtype=np.uint8)
    assert ev.truth_label_values(["label_val_200", "label_val_0", "label_val_7"], truth, 3).tolist() == [0, 7, 200]
    assert ev.truth_label_values({"label_val_0": 0, "label_val_7": 1, "label_val_200": 2}, None, 3).tolist() == [0, 7, 200]
    assert ev.truth_label_values({"fg": 1}, truth, 3).tolist() == [0, 7, 200]            # codes of another form: ascending unique values
    assert ev.truth_label_values(None, truth.astype(np.int32), 4).tolist() == [0, 7, 200]
    assert ev.truth_label_values({}, truth, 2, ignore_label=200).tolist() == [0, 7]
    assert ev.truth_label_values(["label_val_0", "label_val_7"], truth, 3, label_values=[7, 0, 200]).tolist() == [7, 0, 200]   # explicit wins
    with pytest.raises(ValueError, match="3 label values"):
        ev.truth_label_values({}, truth, 2)
    with pytest.raises(ValueError):
        ev.truth_label_values(["label_val_0", "label_val_7", "label_val_200"], truth, 2)


def test_label_values_map_raw_truth_to_class_indices():
    pred, cls = random_pair(3, seed=3)
    raw = np.array([0, 7, 200], dtype=np.uint8)[cls]
    want = ev.confusion_matrix(pred, cls, 3, device="cpu")[0]
    assert np.array_equal(ev.confusion_matrix(pred, raw, 3, label_values=[0, 7, 200], device="cpu")[0], want)
    wide = np.array([-5, 1000, 70000], dtype=np.int64)[cls]                            # wider dtype: mapped on the host
    assert np.array_equal(ev.confusion_matrix(pred, wide, 3, label_values=[-5, 1000, 70000], device="cpu")[0], want)
    assert np.array_equal(ev.confusion_matrix(pred.astype(np.int32), cls.astype(np.uint16), 3, device="cpu")[0], want)


# ---- the NumPy route -----------------------------------------------------------------------------------------------------------
def test_numpy_route_per_slice_ignore_and_invalid():
    pred, truth = random_pair(4, shape=(5, 7, 9), seed=4)
    whole, dropped = ev.confusion_matrix(pred, truth, 4, device="cpu")
    per, dper = ev.confusion_matrix(pred, truth, 4, per_slice=True, device="cpu")
    assert per.shape == (5, 4, 4) and dper.shape == (5, 2) and per.dtype == np.int64
    assert np.array_equal(per.sum(0), whole)
    for s in range(5):
        assert np.array_equal(per[s], np.bincount(truth[s].ravel().astype(np.int64) * 4 + pred[s].ravel(), minlength=16).reshape(4, 4))
    dice = ev.dice_per_slab(per)
    assert dice.shape == (5, 4)
    for s in range(5):
        np.testing.assert_allclose(dice[s], brute_scores(pred[s], truth[s], 4)["dice"], rtol=0, atol=1e-12, equal_nan=True)

    marked = truth.copy()
    marked[1, 2, :4] = 99
    marked[3, 0, 0] = 99
    counts, dropped = ev.confusion_matrix(pred, marked, 4, ignore_label=99, per_slice=True, device="cpu")
    assert dropped[:, 0].tolist() == [0, 4, 0, 1, 0] and dropped[:, 1].sum() == 0
    keep = marked != 99
    assert np.array_equal(counts.sum(0), np.bincount(truth[keep].astype(np.int64) * 4 + pred[keep], minlength=16).reshape(4, 4))

    with pytest.raises(ValueError, match=r"5 of 315 voxels.*ground-truth values \[99\]"):     # the same truth without ignore_label
        ev.confusion_matrix(pred, marked, 4, device="cpu")
    bad = pred.copy()
    bad[0, 0, 0] = 4
    bad[4, 6, 8] = 9
    with pytest.raises(ValueError, match=r"2 of 315 voxels.*prediction values \[4, 9\]"):
        ev.confusion_matrix(bad, truth, 4, device="cpu")
    with pytest.raises(ValueError, match="shape"):
        ev.confusion_matrix(pred[:, :, :8], truth, 4, device="cpu")


# ---- the command, --prediction mode ----------------------------------------------------------------------------------------------
def test_evaluate_command_scores_existing_label_volumes(tmp_path):
    from volume_segmantics_amd.scripts import evaluate_2d_model
    from volume_segmantics_amd.utilities import base_data_utils as utils
    pred, truth = random_pair(3, shape=(4, 10, 12), seed=5)
    raw = np.array([0, 7, 200], dtype=np.uint8)
    utils.save_data_to_hdf5(raw[pred], tmp_path / "pred.h5")
    utils.save_data_to_hdf5(raw[truth], tmp_path / "truth.h5")
    evaluate_2d_model.main(["--prediction", str(tmp_path / "pred.h5"), "--labels", str(tmp_path / "truth.h5"), "--data_dir", str(tmp_path)])
    b = brute_scores(pred, truth, 3)

    doc = json.loads((tmp_path / "pred_scores.json").read_text())
    assert [c["label_value"] for c in doc["classes"]] == [0, 7, 200]
    assert [c["truth_voxels"] for c in doc["classes"]] == b["truth"] and [c["true_positives"] for c in doc["classes"]] == b["tp"]
    assert [c["predicted_voxels"] for c in doc["classes"]] == b["pred"]
    for name in ("dice", "iou", "precision", "recall"):
        np.testing.assert_allclose([c[name] for c in doc["classes"]], b[name], rtol=0, atol=1e-12)
    assert abs(doc["mean_dice"] - b["mean_dice"]) <= 1e-12 and abs(doc["mean_iou"] - b["mean_iou"]) <= 1e-12
    assert abs(doc["accuracy"] - b["accuracy"]) <= 1e-12 and doc["dropped"] == {"ignored": 0, "invalid": 0}
    assert np.array_equal(np.array(doc["confusion_matrix"]), np.bincount(truth.ravel().astype(np.int64) * 3 + pred.ravel(), minlength=9).reshape(3, 3))

    rows = list(csv.reader((tmp_path / "pred_scores.csv").open()))
    assert rows[0] == ["class", "label_value", "truth_voxels", "predicted_voxels", "true_positives", "dice", "iou", "precision", "recall"]
    assert [r[0] for r in rows[1:]] == ["0", "1", "2", "mean", "accuracy"] and [r[1] for r in rows[1:4]] == ["0", "7", "200"]
    for c in range(3):
        assert [int(v) for v in rows[1 + c][2:5]] == [b["truth"][c], b["pred"][c], b["tp"][c]]
        np.testing.assert_allclose([float(v) for v in rows[1 + c][5:9]], [b[n][c] for n in ("dice", "iou", "precision", "recall")], rtol=0, atol=1e-12)
    assert abs(float(rows[4][5]) - b["mean_dice"]) <= 1e-12 and abs(float(rows[4][6]) - b["mean_iou"]) <= 1e-12
    assert abs(float(rows[5][5]) - b["accuracy"]) <= 1e-12
    assert not (tmp_path / "pred_scores_per_slice.csv").exists()


def test_evaluate_command_usage_errors_exit_2(tmp_path):
    from volume_segmantics_amd.scripts import evaluate_2d_model
    np.save(tmp_path / "a.npy", np.zeros((2, 3, 4), dtype=np.uint8))
    (tmp_path / "pred.txt").write_text("x")
    for argv in (["--prediction", str(tmp_path / "pred.txt"), "--labels", str(tmp_path / "a.npy")],      # wrong suffix
                 ["--prediction", str(tmp_path / "missing.npy"), "--labels", str(tmp_path / "a.npy")],   # no such file
                 ["--labels", str(tmp_path / "a.npy")],                                                    # neither form
                 ["--prediction", str(tmp_path / "a.npy")]):                                               # no labels
        with pytest.raises(SystemExit) as e:
            evaluate_2d_model.main(argv + ["--data_dir", str(tmp_path)])
        assert e.value.code == 2, argv
