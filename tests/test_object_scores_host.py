"""The host route of utilities/object_scores.py against a plain-Python oracle, hand-built scenes with known answers, the files, the
evaluate command's --prediction form and the committed vessels digest.  No GPU."""
import csv
import json
import math
from types import SimpleNamespace

import numpy as np
import pytest

import object_score_cases as oc
from volume_segmantics_amd.utilities import object_scores as obs


# ---- the overlap table -----------------------------------------------------------------------------------------------------------------
def test_host_overlap_table_matches_the_oracle():
    for (name, a, b, skip), (want, runs) in zip(oc.sweep_volumes(), oc.sweep_expected()):
        got = obs.overlap_table(a, b, skip, device="cpu")
        oc.assert_tables_equal(got, want, name)
        assert obs.count_runs_host(a, b, skip, a.shape[-1]) == runs >= len(want[0]), name
    names = [name for name, *_ in oc.sweep_volumes()]
    assert len(oc.sweep_expected()[names.index("17x19x67 random K=4")][0][0]) > 2000            # thousands of keys
    assert len(oc.sweep_expected()[names.index("skip everything")][0][0]) == 0
    assert len(oc.sweep_expected()[names.index("two solid volumes")][0][0]) == 1


def test_overlap_table_argument_errors():
    a = np.zeros((2, 3, 4), dtype=np.int32)
    with pytest.raises(ValueError, match="shapes must be equal"):
        obs.overlap_table(a, a[:, :, :3], device="cpu")
    with pytest.raises(ValueError, match="shapes must be equal"):
        obs.overlap_table(a, a, np.zeros((2, 3), dtype=bool), device="cpu")
    with pytest.raises(TypeError, match="int32"):
        obs.overlap_table(a.astype(np.int64), a, device="cpu")
    assert [obs.table_slots(r) for r in (0, 1, 32, 33, 64, 100)] == [64, 64, 64, 128, 128, 256]


# ---- the figures -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", oc.hand_cases(), ids=[c[0] for c in oc.hand_cases()])
def test_hand_built_scenes(case):
    _, pred, truth, kwargs, expected, partition = case
    overlaps = obs.object_overlaps(pred, truth, 2, device="cpu", **kwargs)
    oc.check_hand_case(obs.object_scores_from_overlaps(overlaps), expected, partition)


def test_ignored_object_changes_nothing():
    """the scene with an ignored region scores exactly as the scene without the region and without the object inside it"""
    cases = {c[0]: c for c in oc.hand_cases()}
    _, pred, truth, kwargs, _, _ = cases["an object inside the ignore label"]
    with_region = obs.object_scores_from_overlaps(obs.object_overlaps(pred, truth, 2, device="cpu", **kwargs), background=True)
    plain_truth = np.where(truth == 9, 0, truth)
    plain = obs.object_scores_from_overlaps(obs.object_overlaps(plain_truth, plain_truth, 2, device="cpu"), background=True)
    assert [(c["true_objects"], c["predicted_objects"]) for c in with_region["classes"]] == [(1, 1), (1, 1)]
    for got, want in zip(with_region["classes"], plain["classes"]):
        assert got["thresholds"][0]["tp"] == want["thresholds"][0]["tp"] == 1
    assert with_region["partition"]["voxels"] == truth.size - int((truth == 9).sum())


def test_partition_scores_and_thresholds_against_the_oracle():
    rng = np.random.default_rng(3)
    truth = oc.cc.random_labels((5, 9, 31), 3, 0.4, seed=3)           # sparse enough for many objects of classes 1 and 2
    pred = np.where(rng.random(truth.shape) < 0.1, rng.integers(0, 3, truth.shape, dtype=np.uint8), truth)
    overlaps = obs.object_overlaps(pred, truth, 3, connectivity=6, device="cpu")
    scores = obs.object_scores_from_overlaps(overlaps, iou=[0.5, 0.75], min_voxels=2, background=True)
    split, merge, are = oc.oracle_partition(overlaps["a"], overlaps["b"], overlaps["count"])
    p = scores["partition"]
    assert p["vi_split"] == split and p["vi_merge"] == merge and abs(p["adapted_rand_error"] - are) <= 4e-16 and p["voxels"] == truth.size
    # the counts of every class and threshold, recounted pair by pair from the table
    t = {r: (c, s) for r, c, s in zip(overlaps["truth_roots"].tolist(), overlaps["truth_classes"].tolist(), overlaps["truth_sizes"].tolist())}
    q = {r: (c, s) for r, c, s in zip(overlaps["pred_roots"].tolist(), overlaps["pred_classes"].tolist(), overlaps["pred_sizes"].tolist())}
    assert sum(s for _, s in t.values()) == sum(s for _, s in q.values()) == truth.size
    for c in range(3):
        nt, npred = sum(1 for k, s in t.values() if k == c and s >= 2), sum(1 for k, s in q.values() if k == c and s >= 2)
        assert (scores["classes"][c]["true_objects"], scores["classes"][c]["predicted_objects"]) == (nt, npred) and nt > (1 if c else 0)
        for k, thr in enumerate((0.5, 0.75)):
            ious = [n / (t[a][1] + q[b][1] - n) for a, b, n in zip(overlaps["a"].tolist(), overlaps["b"].tolist(), overlaps["count"].tolist())
                    if t[a][0] == c == q[b][0] and t[a][1] >= 2 and q[b][1] >= 2 and n / (t[a][1] + q[b][1] - n) > thr]
            row = scores["classes"][c]["thresholds"][k]
            assert (row["tp"], row["fp"], row["fn"]) == (len(ious), npred - len(ious), nt - len(ious))
            assert abs(row["pq"] - math.fsum(ious) / (len(ious) + (npred - len(ious)) / 2 + (nt - len(ious)) / 2)) <= 1e-15
        partners = {}
        for a, b in zip(overlaps["a"].tolist(), overlaps["b"].tolist()):
            if t[a][0] == c == q[b][0] and t[a][1] >= 2 and q[b][1] >= 2:
                partners.setdefault(a, set()).add(b)
        assert scores["classes"][c]["splits"] == sum(1 for s in partners.values() if len(s) >= 2)
    assert scores["means"][0]["f1"] == math.fsum(c["thresholds"][0]["f1"] for c in scores["classes"]) / 3
    for bad in (0.4, 1.0, [0.5, 0.2]):
        with pytest.raises(ValueError, match="evaluation_object_iou"):
            obs.object_scores_from_overlaps(overlaps, iou=bad)


def test_settings():
    s = obs.object_settings(SimpleNamespace())
    assert s == dict(active=False, connectivity=6, iou=[0.5], min_voxels=1, min_overlap=1, background=False)
    s = obs.object_settings(SimpleNamespace(evaluation_object_scores=True, postprocess_connectivity=18, evaluation_object_iou=[0.5, 0.9]))
    assert s["active"] and s["connectivity"] == 18 and s["iou"] == [0.5, 0.9]
    assert obs.object_settings(SimpleNamespace(postprocess_connectivity=18, evaluation_object_connectivity=26))["connectivity"] == 26
    with pytest.raises(ValueError, match="6, 18 or 26"):
        obs.object_settings(SimpleNamespace(evaluation_object_connectivity=8))
    # an evaluation that does not ask for object scores never reads the other keys
    assert not obs.object_scores_asked(SimpleNamespace(evaluation_object_connectivity=8, evaluation_object_iou=0.2))
    assert obs.object_scores_asked(SimpleNamespace(evaluation_object_scores=True))


def test_evaluate_command_ignores_bad_object_keys_when_not_asked(tmp_path):
    from volume_segmantics_amd.scripts import evaluate_2d_model
    from volume_segmantics_amd.utilities import base_data_utils as utils
    (tmp_path / "volseg-settings").mkdir()
    (tmp_path / "volseg-settings" / "2d_model_predict_settings.yaml").write_text("evaluation_object_iou: 0.2\nevaluation_object_connectivity: 8\n")
    vol = np.zeros((2, 3, 4), dtype=np.uint8)
    vol[0, 1, 1:3] = 1
    utils.save_data_to_hdf5(vol, tmp_path / "pred.h5")
    utils.save_data_to_hdf5(vol, tmp_path / "truth.h5")
    evaluate_2d_model.main(["--prediction", str(tmp_path / "pred.h5"), "--labels", str(tmp_path / "truth.h5"), "--data_dir", str(tmp_path)])
    assert (tmp_path / "pred_scores.json").exists() and not (tmp_path / "pred_object_scores.json").exists()


# ---- the files ---------------------------------------------------------------------------------------------------------------------
def test_files(tmp_path):
    cases = {c[0]: c for c in oc.hand_cases()}
    _, pred, truth, _, _, _ = cases["split, larger piece matches"]
    pred = pred.copy()
    pred[3, 4, 15:20] = 1                                              # an invented object as well
    settings = SimpleNamespace(evaluation_object_scores=True, evaluation_object_iou=[0.5, 0.8])
    raw = np.array([0, 7, 200], dtype=np.uint8)                        # the truth holds label values, the prediction class indices; class 2 is absent
    scores, _ = obs.evaluate_objects(pred, raw[truth], 3, settings, label_values=raw, device="cpu", stem=tmp_path / "seg")
    assert sorted(p.name for p in tmp_path.iterdir()) == ["seg_object_matches.csv", "seg_object_scores.csv", "seg_object_scores.json"]

    text = (tmp_path / "seg_object_scores.json").read_text()
    assert "NaN" not in text
    doc = json.loads(text)
    assert doc["settings"] == dict(iou=[0.5, 0.8], min_voxels=1, min_overlap=1, background=False, connectivity=6)
    assert [c["label_value"] for c in doc["classes"]] == [0, 7, 200]
    assert doc["classes"][2]["thresholds"][0]["f1"] is None and doc["classes"][2]["splits"] is None             # NaN is written as null
    one = doc["classes"][1]
    assert (one["true_objects"], one["predicted_objects"], one["splits"], one["merges"]) == (1, 3, 1, 0)
    assert [(r["tp"], r["fp"], r["fn"]) for r in one["thresholds"]] == [(1, 2, 0), (0, 3, 1)]
    assert one["thresholds"][0]["pq"] == 0.7 / 2 and one["thresholds"][1]["sq"] is None
    # the round trip: the document holds what the scores hold, NaN as null
    for got, want in zip(doc["classes"], scores["classes"]):
        for g, w in zip(got["thresholds"], want["thresholds"]):
            assert all((g[k] is None and math.isnan(w[k])) or g[k] == w[k] for k in w)
    assert doc["partition"] == {k: v for k, v in scores["partition"].items()} and doc["means"][0]["f1"] == scores["means"][0]["f1"]

    rows = list(csv.reader((tmp_path / "seg_object_scores.csv").open()))
    assert tuple(rows[0]) == obs.SCORE_COLUMNS and len(rows) == 1 + 3 * 2 + 2 and [r[0] for r in rows[-2:]] == ["mean", "mean"]
    assert rows[3][:8] == ["1", "7", "0.5", "1", "3", "1", "2", "0"] and float(rows[3][8]) == 1 / 3 and rows[5][12] == "nan"

    rows = list(csv.reader((tmp_path / "seg_object_matches.csv").open()))
    assert tuple(rows[0]) == obs.MATCH_COLUMNS and len(rows) == 1 + 1 + 2
    assert rows[1] == ["1", "7", "1", "2", "2", "10", "1", "2", "2", "7", "7", "0.7", "1", "2"]
    assert [r[:6] for r in rows[2:]] == [["1", "7", "", "", "", ""]] * 2 and [r[6:10] for r in rows[2:]] == [["1", "2", "10", "2"], ["3", "4", "15", "5"]]


# ---- the command, --prediction mode ------------------------------------------------------------------------------------------------------
def test_evaluate_command_object_scores(tmp_path):
    from volume_segmantics_amd.scripts import evaluate_2d_model
    from volume_segmantics_amd.utilities import base_data_utils as utils
    cases = {c[0]: c for c in oc.hand_cases()}
    _, pred, truth, _, expected, _ = cases["two objects bridged"]
    raw = np.array([0, 200], dtype=np.uint8)
    runs = {}
    for name, extra in (("off", ""), ("on", "evaluation_object_scores: true\nevaluation_object_iou: [0.5, 0.7]\n")):
        root = tmp_path / name
        (root / "volseg-settings").mkdir(parents=True)
        (root / "volseg-settings" / "2d_model_predict_settings.yaml").write_text("evaluation_per_slice: true\n" + extra)
        utils.save_data_to_hdf5(raw[pred], root / "pred.h5")
        utils.save_data_to_hdf5(raw[truth], root / "truth.h5")
        before = {p.name for p in root.iterdir()}
        evaluate_2d_model.main(["--prediction", str(root / "pred.h5"), "--labels", str(root / "truth.h5"), "--data_dir", str(root)])
        runs[name] = {p.name: p.read_bytes() for p in root.iterdir() if p.name not in before}
    today = {"pred_scores.csv", "pred_scores.json", "pred_scores_per_slice.csv"}
    assert set(runs["off"]) == today
    assert set(runs["on"]) == today | {"pred_object_scores.csv", "pred_object_scores.json", "pred_object_matches.csv"}
    for name in today:
        assert runs["on"][name] == runs["off"][name], name
    doc = json.loads(runs["on"]["pred_object_scores.json"])
    one = doc["classes"][1]
    assert one["label_value"] == 200 and (one["true_objects"], one["predicted_objects"], one["merges"]) == (2, 1, 1)
    assert [(r["tp"], r["fp"], r["fn"]) for r in one["thresholds"]] == [(0, 1, 2)] * 2


# ---- the vessels digest ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", list(oc.VESSELS_RUNS))
def test_vessels_digest(run):
    pred, truth = oc.vessels_pair()
    if oc.VESSELS_RUNS[run]["swapped"]:
        pred, truth = truth, pred
    overlaps = obs.object_overlaps(pred, truth, 2, connectivity=oc.VESSELS_RUNS[run]["connectivity"], device="cpu")
    got = oc.vessels_digest(overlaps, obs.object_scores_from_overlaps(overlaps))
    assert got == oc.vessels_expected()[run]
    # the integers the pair was first checked with (scipy.ndimage.label of the foreground)
    known = {"connectivity_6": dict(true_objects=15, predicted_objects=44, table_rows_one_background=102, tp=13, fp=31, fn=2, splits=7, merges=0,
                                    runs=673186),
             "connectivity_6_swapped": dict(merges=7),
             "connectivity_26": dict(true_objects=14, predicted_objects=41, table_rows_one_background=96, tp=12, splits=6)}[run]
    assert {k: got[k] for k in known} == known
