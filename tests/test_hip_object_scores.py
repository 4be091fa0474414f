"""-m gpu: the kernels of csrc/overlap.hip - vs_overlap_runs, vs_overlap_table - bit for bit against the host route and the plain-Python
oracle of tests/object_score_cases.py at the sizes where the sweep can go wrong, the error path of a table that is too small,
the hand-built scenes and the vessels digest through the device route, and VolSeg2DPredictionManager.evaluate_volume with
evaluation_object_scores.  Output buffers start out full of garbage (torch.empty)."""
import json
from types import SimpleNamespace

import numpy as np
import pytest

import object_score_cases as oc
from volume_segmantics_amd.utilities import object_scores as obs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_device_overlap_table_matches_host_and_oracle():
    import torch
    for (name, a, b, skip), (want, runs) in zip(oc.sweep_volumes(), oc.sweep_expected()):
        got = obs.overlap_table(a, b, skip, device=DEV)
        oc.assert_tables_equal(got, want, name)
        oc.assert_tables_equal(got, obs.overlap_table(a, b, skip, device="cpu"), name)
        oc.assert_tables_equal(obs.overlap_table(a, b, skip, device=DEV), got, name + ", again")            # two calls, the same sorted table
        oc.assert_tables_equal(obs.overlap_table_unique(a, b, skip, device=DEV), want, name + ", torch.unique")
        da, db, ds = obs.device_inputs(a.reshape(-1), b.reshape(-1), None if skip is None else skip.reshape(-1), torch.device(DEV))
        got_runs = obs.runs_device(da, db, ds, a.shape[-1])
        assert got_runs == runs == obs.count_runs_host(a, b, skip, a.shape[-1]) and got_runs >= len(want[0]), name
        # resident tensors are taken as they are
        oc.assert_tables_equal(obs.overlap_table(da.reshape(a.shape), db.reshape(a.shape), None if ds is None else ds.reshape(a.shape)), want, name)


def test_table_too_small_is_an_error_not_a_spin():
    """about a hundred keys into 4 slots: every probe loop ends after 4 steps, the call returns the error code and names the table size"""
    import torch
    from volume_segmantics_amd import _lib
    a, b = oc.hundred_keys()
    assert len(oc.oracle_table(a, b)[0][0]) == 112
    da, db, _ = obs.device_inputs(a.reshape(-1), b.reshape(-1), None, torch.device(DEV))
    keys, counts = (torch.empty(4, dtype=torch.int64, device=DEV) for _ in range(2))
    used = torch.empty(2, dtype=torch.int64, device=DEV)
    with torch.cuda.device(DEV):
        rc = _lib.lib.vs_overlap_table(_lib.ptr(da), _lib.ptr(db), None, da.numel(), a.shape[-1], _lib.ptr(keys), _lib.ptr(counts), 4, _lib.ptr(used),
                                       _lib.stream_ptr())
    assert rc == -1 and "4 slots" in _lib.last_error() and used.cpu().tolist() == [4, 1]            # VS_ERR_INVALID
    with pytest.raises(RuntimeError, match="4 slots"):
        obs.hash_device(da, db, None, a.shape[-1], 4)
    with pytest.raises(RuntimeError, match="power of two"):
        obs.hash_device(da, db, None, a.shape[-1], 96)
    # the same volume with room: the device is fine and so is the table
    oc.assert_tables_equal(obs.overlap_table(a, b, device=DEV), oc.oracle_table(a, b)[0])


@pytest.mark.parametrize("case", oc.hand_cases(), ids=[c[0] for c in oc.hand_cases()])
def test_hand_built_scenes_on_the_device(case):
    _, pred, truth, kwargs, expected, partition = case
    overlaps = obs.object_overlaps(pred, truth, 2, device=DEV, **kwargs)
    host = obs.object_overlaps(pred, truth, 2, device="cpu", **kwargs)
    assert sorted(overlaps) == sorted(host)
    for key in host:
        assert np.array_equal(overlaps[key], host[key]), key
    oc.check_hand_case(obs.object_scores_from_overlaps(overlaps), expected, partition)


@pytest.mark.parametrize("run", list(oc.VESSELS_RUNS))
def test_vessels_digest_on_the_device(run):
    pred, truth = oc.vessels_pair()
    if oc.VESSELS_RUNS[run]["swapped"]:
        pred, truth = truth, pred
    overlaps = obs.object_overlaps(pred, truth, 2, connectivity=oc.VESSELS_RUNS[run]["connectivity"], device=DEV)
    assert oc.vessels_digest(overlaps, obs.object_scores_from_overlaps(overlaps)) == oc.vessels_expected()[run]


def test_evaluate_volume_with_object_scores(tmp_path):
    """a stub-predicted 9 x 10 x 70 volume against a truth with label values and an ignored region"""
    from volume_segmantics_amd.model.operations import vol_seg_prediction_manager as pm
    truth_classes = oc.cc.random_labels((9, 10, 70), 3, 0.4, seed=5)
    rng = np.random.default_rng(6)
    labels = np.where(rng.random(truth_classes.shape) < 0.1, rng.integers(0, 3, truth_classes.shape, dtype=np.uint8), truth_classes).astype(np.uint8)
    truth = np.array([0, 7, 200], dtype=np.uint8)[truth_classes]
    truth[2:5, 3:8, 20:50] = 255
    fake = SimpleNamespace(_predict_single_axis=lambda vol, axis: (labels, None), model_device_num=0, num_labels=3, label_codes={})
    settings = SimpleNamespace(one_hot=False, quality="low", prediction_axis="Z", output_probs=False, evaluation_ignore_label=255,
                               postprocess_connectivity=18)
    manager = pm.VolSeg2DPredictionManager.__new__(pm.VolSeg2DPredictionManager)
    manager.predictor, manager.settings, manager.data_vol, manager.input_data_chunking, manager.downsample = fake, settings, labels, True, False

    (tmp_path / "off").mkdir()
    (tmp_path / "on").mkdir()
    plain = manager.evaluate_volume(truth, tmp_path / "off" / "seg.h5")
    assert "object_scores" not in manager.last_evaluation
    assert sorted(p.name for p in (tmp_path / "off").iterdir()) == ["seg.h5", "seg_scores.csv", "seg_scores.json"]           # the key absent: as before

    settings.evaluation_object_scores = True
    settings.evaluation_object_iou = [0.5, 0.75]
    scores = manager.evaluate_volume(truth, tmp_path / "on" / "seg.h5")
    assert np.array_equal(scores.confusion, plain.confusion)
    assert sorted(p.name for p in (tmp_path / "on").iterdir()) == ["seg.h5", "seg_object_matches.csv", "seg_object_scores.csv", "seg_object_scores.json",
                                                                    "seg_scores.csv", "seg_scores.json"]
    for name in ("seg.h5", "seg_scores.csv", "seg_scores.json"):
        assert (tmp_path / "on" / name).read_bytes() == (tmp_path / "off" / name).read_bytes(), name

    got = manager.last_evaluation["object_scores"]
    host_overlaps = obs.object_overlaps(labels, truth, 3, label_values=[0, 7, 200], ignore_label=255, connectivity=18, device="cpu")      # connectivity from postprocess_connectivity
    want = obs.object_scores_from_overlaps(host_overlaps, iou=[0.5, 0.75])
    want["settings"]["connectivity"] = 18
    assert json.dumps(obs.json_ready(got), sort_keys=True) == json.dumps(obs.json_ready(want), sort_keys=True)
    assert got["classes"][1]["true_objects"] > 1 and got["classes"][1]["thresholds"][0]["tp"] > 0
    assert got["partition"]["voxels"] == truth.size - 3 * 5 * 30
    doc = json.loads((tmp_path / "on" / "seg_object_scores.json").read_text())
    assert doc["classes"][1]["label_value"] == 7 and doc["classes"][1]["thresholds"][0]["tp"] == got["classes"][1]["thresholds"][0]["tp"]
