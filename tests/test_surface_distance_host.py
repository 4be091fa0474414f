"""Surface distances, the host side (utilities/surface_distance.py, the evaluate command with evaluation_surface_distances): the
oracles of tests/surface_cases.py against each other, the C ABI of csrc/surface.hip, every function's host route against the
oracles, the figures against np.percentile / mean / max on explicit distance arrays, and the command on existing label volumes.
The HIP kernels themselves: tests/test_hip_surface_distance.py."""
import csv
import ctypes
import json
import re
from pathlib import Path

import numpy as np
import pytest

import surface_cases as sc
from volume_segmantics_amd.utilities import surface_distance as sd

REPO = Path(__file__).resolve().parent.parent


# ---- the oracles -------------------------------------------------------------------------------------------------------------------
def test_minplus_oracle_equals_brute_force_and_scipy():
    seeds = np.random.default_rng(0).random((5, 7, 9)) < 0.3
    want = sc.brute_d2(seeds)
    assert want.dtype == np.uint32 and want[seeds].max() == 0 and want[~seeds].min() >= 1
    assert np.array_equal(sc.minplus_d2(seeds), want)
    assert (sc.minplus_d2(np.zeros((2, 3, 4), bool)) == sc.INF).all() and (sc.brute_d2(np.zeros((2, 3, 4), bool)) == sc.INF).all()
    ndimage = pytest.importorskip("scipy.ndimage")
    assert np.array_equal(np.rint(ndimage.distance_transform_edt(~seeds) ** 2).astype(np.uint32), want)


# ---- C ABI -------------------------------------------------------------------------------------------------------------------------
def test_surface_entry_points_are_declared_exported_and_bound():
    from volume_segmantics_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "volseg_hip.h").read_text(), flags=re.S)
    exported = ctypes.CDLL(str(_lib.LIB_PATH))
    I, I64, P, SZ = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_size_t
    want = {"vs_label_surface": (I, [P, P, I, I64, I64, I64, P, P, P]),
            "vs_edt_workspace_bytes": (SZ, [I64, I64, I64]),
            "vs_edt_squared": (I, [P, I64, I64, I64, P, P, SZ, P]),
            "vs_surface_distance_histogram": (I, [P, P, I64, I64, P, P])}
    for name, (res, args) in want.items():
        ret = "size_t" if res is SZ else "int"
        found = re.search(rf"\b{ret}\s+{name}\s*\(([^)]*)\)", header)
        assert found, name
        assert len(found.group(1).split(",")) == len(args), name
        assert hasattr(exported, name), name
        assert _lib._SIGS[name] == (res, args), name
        fn = getattr(_lib.lib, name)
        assert fn.restype is res and fn.argtypes == args, name
    source = (REPO / "volume-segmantics_amd" / "csrc" / "surface.hip").read_text()
    assert int(re.search(r"kMaxLdsAxis\s*=\s*(\d+)", source).group(1)) == sd.EDT_LDS_MAX_AXIS


# ---- host routes against the oracles --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,density", [((5, 7, 9), 0.3), ((3, 20, 17), 0.02), ((1, 13, 11), 0.1), ((14,), 0.2), ((6, 5), 0.2)])
def test_squared_distance_transform_host(shape, density, monkeypatch):
    seeds = np.random.default_rng(len(shape)).random(shape) < density
    want = sc.brute_d2(seeds)
    got = sd.squared_distance_transform(seeds, device="cpu")
    assert got.dtype == np.uint32 and got.shape == shape and np.array_equal(got, want)
    assert np.array_equal(sd.squared_distance_transform(seeds.astype(np.int32) * 7, device="cpu"), want)
    import builtins
    real_import = builtins.__import__

    def no_scipy(name, *args, **kwargs):
        if name.split(".")[0] == "scipy":
            raise ImportError(name)
        return real_import(name, *args, **kwargs)

    monkeypatch.setattr(builtins, "__import__", no_scipy)          # the NumPy min-plus route of a host without scipy
    assert np.array_equal(sd.squared_distance_transform(seeds, device="cpu"), want)
    assert (sd.squared_distance_transform(np.zeros(shape, np.uint8), device="cpu") == sc.INF).all()


def test_extents_beyond_the_uint32_bound_are_an_error():
    with pytest.raises(ValueError, match="2\\^32"):
        sd.histogram_bins((1, 1, 70000))
    assert sd.histogram_bins((1, 1, 65536)) == 65535 ** 2 + 2 and sd.histogram_bins((12, 24, 40)) == 11 ** 2 + 23 ** 2 + 39 ** 2 + 2


def test_label_surface_host():
    pred, truth = sc.coherent_pair()
    for c in range(4):
        got = sd.label_surface(truth, c, device="cpu")
        assert got.dtype == np.uint8 and np.array_equal(got, sc.surface_np(truth == c))
    raw = np.array([0, 7, 100, 200], dtype=np.uint8)[truth]
    raw[:, 10:12, :] = 255
    ignored = raw == 255
    for c in range(4):
        want = sc.surface_np((truth == c) & ~ignored)
        assert np.array_equal(sd.label_surface(raw, c, label_values=[0, 7, 100, 200], ignore_label=255, device="cpu"), want)
        wide = np.array([-5, 1000, 70000, 9], dtype=np.int64)[truth]
        wide[ignored] = -1
        assert np.array_equal(sd.label_surface(wide, c, label_values=[-5, 1000, 70000, 9], ignore_label=-1, device="cpu"), want)
    flat = truth[:1]
    assert np.array_equal(sd.label_surface(flat, 2, device="cpu"), sc.surface_np(flat == 2))
    assert np.array_equal(sd.label_surface(flat[0], 2, device="cpu"), sc.surface_np(flat[0] == 2))     # 1 x H x W: the 2-D surface
    full = sd.label_surface(np.full((4, 5, 6), 3, np.uint8), 3, device="cpu")
    assert full.sum() == 4 * 5 * 6 - 2 * 3 * 4 and full[1:-1, 1:-1, 1:-1].sum() == 0
    assert sd.label_surface(truth, 9, device="cpu").sum() == 0


def test_histograms_host_equal_the_oracle():
    pred, truth = sc.coherent_pair()
    want, want_inf = sc.coherent_reference()
    got, inf = sd.surface_distance_histograms(pred, truth, 4, device="cpu")
    assert got.dtype == np.int64 and inf.dtype == np.int64
    assert np.array_equal(got, want) and np.array_equal(inf, want_inf) and inf.sum() == 0
    assert got[:, :, :2].sum() > 0.9 * got.sum()                   # a coherent pair: nearly all surface voxels coincide or are one voxel off
    assert got[:, :, -1].any()                                     # trailing all-zero bins are trimmed
    sub, sub_inf = sd.surface_distance_histograms(pred, truth, [2, 0], device="cpu")
    assert np.array_equal(sub[:, :, :], want[[2, 0]][:, :, :sub.shape[2]]) and not want[[2, 0]][:, :, sub.shape[2]:].any()
    for p, t in ((pred.astype(np.int32), truth.astype(np.int64)), (pred.astype(np.uint16), truth)):       # wide integer dtypes
        g, i = sd.surface_distance_histograms(p, t, 4, device="cpu")
        assert np.array_equal(g, want) and np.array_equal(i, want_inf)
    with pytest.raises(ValueError, match="shape"):
        sd.surface_distance_histograms(pred[:, :, :-1], truth, 4, device="cpu")


def test_absent_classes_ignore_label_label_values_and_flat_volumes():
    pred, truth = (a.copy() for a in sc.coherent_pair())
    pred[pred == 3] = 2                                            # class 3: in the truth only; class 4: in neither
    hists, inf = sd.surface_distance_histograms(pred, truth, 5, device="cpu")
    want, want_inf = sc.histograms_np(pred, truth, 5)
    assert np.array_equal(hists, want) and np.array_equal(inf, want_inf)
    surface_a = int(sc.surface_np(truth == 3).sum())
    assert inf[3].tolist() == [surface_a, 0] and surface_a > 0 and not hists[3].any() and not hists[4].any() and inf[4].tolist() == [0, 0]
    s = sd.surface_scores_from_histograms(hists, inf)
    for name in sc.FLOAT_FIGURES:
        assert np.isinf(getattr(s, name)[3]) and np.isnan(getattr(s, name)[4]), name
    assert s.surface_dice[3] == 0.0 and np.isnan(s.surface_dice[4])
    assert s.truth_surface_voxels[3] == surface_a and s.predicted_surface_voxels[3] == 0
    assert np.isinf(s.mean_hausdorff) and abs(s.mean_surface_dice - s.surface_dice[:4].mean()) <= 1e-15
    sc.assert_surface_scores_equal(s, sc.brute_surface_scores(pred, truth, 5))

    pred, truth = sc.coherent_pair()
    raw = np.array([0, 7, 100, 200], dtype=np.uint8)[truth]
    raw[:, 10:12, :] = 255
    ignored = raw == 255
    want, want_inf = sc.histograms_np(pred, truth, 4, ignored)
    got, inf = sd.surface_distance_histograms(pred, raw, 4, label_values=[0, 7, 100, 200], ignore_label=255, device="cpu")
    assert np.array_equal(got, want) and np.array_equal(inf, want_inf)
    assert not np.array_equal(want[:, :, :3], sc.coherent_reference()[0][:, :, :3])         # the band changes the surfaces

    flat_p, flat_t = pred[:1], truth[:1]                           # 1 x H x W: 2-D surfaces, 2-D distances
    want, want_inf = sc.histograms_np(flat_p[0], flat_t[0], 4, d2=sc.brute_d2)
    got, inf = sd.surface_distance_histograms(flat_p, flat_t, 4, device="cpu")
    assert np.array_equal(got, want) and np.array_equal(inf, want_inf)


# ---- the figures -------------------------------------------------------------------------------------------------------------------
def test_scores_against_explicit_distance_arrays():
    pred, truth = sc.coherent_pair()
    hists, inf = sc.coherent_reference()
    s = sd.surface_scores_from_histograms(hists, inf)
    b = sc.brute_surface_scores(pred, truth, 4)
    sc.assert_surface_scores_equal(s, b)
    assert s.classes == 4 and s.tolerance == 1.0 and s.voxel_size == 1.0
    assert (s.hausdorff >= s.hausdorff_95).all() and (s.hausdorff_95 >= 0).all() and (s.hausdorff > 1).any()
    assert s.truth_surface_voxels.tolist() == hists[:, 0].sum(1).tolist()

    half = sd.surface_scores_from_histograms(hists, inf, tolerance=1.0, voxel_size=0.5)
    sc.assert_surface_scores_equal(half, sc.brute_surface_scores(pred, truth, 4, 1.0, 0.5))
    np.testing.assert_allclose(half.hausdorff, 0.5 * s.hausdorff, rtol=1e-15)
    np.testing.assert_allclose(half.assd, 0.5 * s.assd, rtol=1e-12)
    assert (half.truth_within_tolerance >= s.truth_within_tolerance).all() and (half.surface_dice > s.surface_dice).any()   # d <= 2 voxels now

    wide = sd.surface_scores_from_histograms(hists, inf, tolerance=2.0)
    sc.assert_surface_scores_equal(wide, sc.brute_surface_scores(pred, truth, 4, 2.0, 1.0))
    assert wide.truth_within_tolerance.tolist() == half.truth_within_tolerance.tolist()      # s * d <= 1 with s = 0.5 is d <= 2
    assert np.array_equal(wide.hausdorff, s.hausdorff) and np.array_equal(wide.assd, s.assd)


def test_percentile_of_tiny_multisets():
    for counts in ([1], [1, 1], [3, 0, 0, 1], [19, 1], [20, 1], [1, 0, 0, 0, 0, 39]):
        h = np.zeros((1, 2, len(counts)), dtype=np.int64)
        h[0, 0] = counts
        h[0, 1, 0] = 1                                             # the other direction must be non-empty
        values = np.sqrt(np.repeat(np.arange(len(counts)), counts).astype(np.float64))
        pooled = np.concatenate([values, [0.0]])
        s = sd.surface_scores_from_histograms(h, np.zeros((1, 2), np.int64))
        np.testing.assert_allclose(s.hausdorff_95[0], np.percentile(pooled, 95), rtol=1e-10, atol=0)
        np.testing.assert_allclose(s.assd[0], pooled.mean(), rtol=1e-10, atol=0)
        assert s.hausdorff[0] == pooled.max()


# ---- the command, --prediction mode ----------------------------------------------------------------------------------------------------
def test_evaluate_command_surface_scores(tmp_path):
    from volume_segmantics_amd.scripts import evaluate_2d_model
    from volume_segmantics_amd.utilities import base_data_utils as utils
    pred, truth = sc.coherent_pair((6, 14, 20), seed=3, flips=10)
    raw = np.array([0, 7, 100, 200], dtype=np.uint8)
    runs = {}
    for name, extra in (("off", ""), ("on", "evaluation_surface_distances: true\nevaluation_surface_tolerance: 2.0\nevaluation_voxel_size: 0.5\n")):
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
    assert set(runs["on"]) == today | {"pred_surface_scores.csv", "pred_surface_scores.json"}
    for name in today:
        assert runs["on"][name] == runs["off"][name], name

    b = sc.brute_surface_scores(pred, truth, 4, tolerance=2.0, voxel_size=0.5)
    hists, inf = sc.histograms_np(pred, truth, 4)
    doc = json.loads(runs["on"]["pred_surface_scores.json"])
    assert doc["surface_tolerance"] == 2.0 and doc["voxel_size"] == 0.5
    assert [c["label_value"] for c in doc["classes"]] == [0, 7, 100, 200]
    for name in sc.INTEGER_FIGURES:
        assert [c[name] for c in doc["classes"]] == b[name], name
    for name in sc.FLOAT_FIGURES:
        np.testing.assert_allclose([c[name] for c in doc["classes"]], b[name], rtol=1e-10, atol=0, err_msg=name)
    np.testing.assert_allclose([c["surface_dice"] for c in doc["classes"]], b["surface_dice"], rtol=0, atol=1e-15)
    np.testing.assert_allclose(doc["mean_assd"], b["mean_assd"], rtol=1e-10)
    np.testing.assert_allclose(doc["mean_surface_dice"], b["mean_surface_dice"], rtol=0, atol=1e-15)
    for c in range(4):
        for d, direction in enumerate(("truth_to_pred", "pred_to_truth")):
            h = doc["classes"][c]["histograms"][direction]
            dense = np.zeros(hists.shape[2], dtype=np.int64)
            dense[h["squared_distance"]] = h["count"]
            assert np.array_equal(dense, hists[c, d]) and h["unreached"] == inf[c, d] and all(v > 0 for v in h["count"])

    rows = list(csv.reader(runs["on"]["pred_surface_scores.csv"].decode().splitlines()))
    assert rows[0][:4] == ["class", "label_value", "truth_surface_voxels", "predicted_surface_voxels"]
    assert [r[0] for r in rows[1:]] == ["0", "1", "2", "3", "mean"]
    col = {name: rows[0].index(name) for name in rows[0]}
    for c in range(4):
        assert int(rows[1 + c][col["truth_surface_voxels"]]) == b["truth_surface_voxels"][c]
        np.testing.assert_allclose(float(rows[1 + c][col["hausdorff_95"]]), b["hausdorff_95"][c], rtol=1e-10)
        np.testing.assert_allclose(float(rows[1 + c][col["surface_dice"]]), b["surface_dice"][c], rtol=0, atol=1e-15)
    np.testing.assert_allclose(float(rows[5][col["hausdorff"]]), b["mean_hausdorff"], rtol=1e-10)


def test_json_writes_nan_as_null_and_infinity_as_a_string(tmp_path):
    pred, truth = (a.copy() for a in sc.coherent_pair((4, 9, 11), seed=5, flips=5))
    pred[pred == 3] = 2
    hists, inf = sd.surface_distance_histograms(pred, truth, 5, device="cpu")
    s = sd.surface_scores_from_histograms(hists, inf)
    written = sd.write_surface_scores(tmp_path / "x", s, hists, inf)
    assert [p.name for p in written] == ["x_surface_scores.csv", "x_surface_scores.json"]
    text = written[1].read_text()
    assert "NaN" not in text and "Infinity" not in text
    doc = json.loads(text)
    assert doc["classes"][3]["hausdorff"] == "inf" and doc["classes"][3]["surface_dice"] == 0.0 and doc["mean_assd"] == "inf"
    assert doc["classes"][4]["hausdorff"] is None and doc["classes"][4]["surface_dice"] is None
    assert doc["classes"][3]["histograms"]["truth_to_pred"]["unreached"] == int(inf[3, 0]) > 0
