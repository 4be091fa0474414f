"""Per-class loss weights (settings key `loss_class_weights`), the parts that need no GPU: the settings rules, the balanced counts on
the slicers, the criteria the trainer builds on the CPU route, and the weighted restatements of data/losses.py and of
tests/class_weight_cases.py against the reference project's DiceLoss(weight=...) (tests/golden/g11_weighted_losses.npz, written by
tools/gen_weighted_loss_golden.py) and torch's own BCEWithLogitsLoss(weight) and CrossEntropyLoss(weight, ignore_index)."""
import logging
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from torch import nn

import class_weight_cases as W
import sparse_label_cases as S
import training_scalar_cases as T
import volume_feed_cases as V

# both sides are float64 sums of the same O(1) terms in different orders: at most n k h w = 9207 terms, 1e-16 each
F64_BOUND = 1e-11
KEY = "loss_class_weights"


# ---- settings ----------------------------------------------------------------------------------------------------------------------
def test_a_list_is_rescaled_to_sum_k_and_logged_once(caplog):
    from volume_segmantics_amd.data.losses import resolve_class_weights
    with caplog.at_level(logging.INFO):
        w = resolve_class_weights([1, 3, 4], 3)
    assert w == pytest.approx([3 / 8, 9 / 8, 12 / 8], rel=1e-15) and abs(sum(w) - 3) <= 1e-15
    lines = [r.getMessage() for r in caplog.records if KEY in r.getMessage()]
    assert len(lines) == 1 and "[1.0, 3.0, 4.0]" in lines[0] and "0.375" in lines[0]
    assert resolve_class_weights((2.0, 2.0), 2) == [1.0, 1.0]
    assert resolve_class_weights(None, 3) is None


@pytest.mark.parametrize("spec,word", [([1, 2], "3 classes"), ([1, 2, 3, 4], "3 classes"), ([1, 0, 2], "> 0"), ([1, -2, 3], "> 0"),
                                       ([1, float("nan"), 2], "finite"), ([1, float("inf"), 2], "finite"), ("balance", "not valid"),
                                       ("inverse", "not valid"), (["a", 1, 2], "not valid"), (2.0, "not valid")])
def test_anything_but_k_finite_positive_numbers_is_refused(spec, word):
    from volume_segmantics_amd.data.losses import resolve_class_weights
    with pytest.raises(ValueError, match=KEY) as err:
        resolve_class_weights(spec, 3)
    assert word in str(err.value)


def test_unresolved_balanced_and_the_generalised_dice_are_refused():
    from volume_segmantics_amd.data.losses import HipSegLoss, resolve_class_weights
    with pytest.raises(ValueError, match="unresolved"):
        resolve_class_weights("balanced", 2)
    with pytest.raises(ValueError, match="GeneralizedDiceLoss"):
        resolve_class_weights([1, 1], 2, "GeneralizedDiceLoss")
    with pytest.raises(ValueError, match="GeneralizedDiceLoss"):
        HipSegLoss("GeneralizedDiceLoss", weight=torch.ones(2))
    assert HipSegLoss("GeneralizedDiceLoss").weight is None


# ---- balanced counts ---------------------------------------------------------------------------------------------------------------
def test_class_counts_leave_the_ignore_value_out_and_sum_over_slicers(caplog):
    from volume_segmantics_amd.data import TrainingDataSlicer
    from volume_segmantics_amd.model.operations.vol_seg_2d_trainer import resolve_balanced_class_weights
    slicers, totals = [], np.zeros(3, np.int64)
    for seed, (ignore, classes) in enumerate(((9, (0, 3, 7)), (9, (0, 3, 7)))):
        data, labels = S.sparse_volume(ignore=ignore, classes=classes, seed=seed)
        want = np.array([(labels == c).sum() for c in classes])
        slicer = TrainingDataSlicer(data, labels.copy(), V.settings(ignore_label=ignore))
        assert np.array_equal(slicer.class_counts, want) and slicer.class_counts.sum() == (labels != ignore).sum()
        totals += want
        slicers.append(slicer)
    settings = V.settings(ignore_label=9, **{KEY: "balanced"})
    with caplog.at_level(logging.INFO):
        resolved = resolve_balanced_class_weights(settings, slicers, 3)
    assert getattr(settings, KEY) == "balanced"                              # the caller's settings are left as they were
    w = np.array(getattr(resolved, KEY))
    want = totals.sum() / (3 * totals.astype(np.float64))
    assert np.allclose(w, want * 3 / want.sum(), rtol=1e-14, atol=0) and abs(w.sum() - 3) <= 1e-14
    assert any(str(totals.tolist()) in r.getMessage() for r in caplog.records)
    # without an ignore label: every voxel counts
    data, labels = V.volume_pair((6, 7, 8), "three_classes", 1)
    dense = TrainingDataSlicer(data, labels.copy(), V.settings())
    assert np.array_equal(dense.class_counts, np.bincount(labels.reshape(-1), minlength=3))
    # a list, or no key, passes through untouched
    plain = V.settings(**{KEY: [1, 2, 3]})
    assert resolve_balanced_class_weights(plain, [dense], 3) is plain
    assert resolve_balanced_class_weights(V.settings(), [dense], 3).__dict__ == V.settings().__dict__


def test_balanced_with_a_class_absent_is_refused():
    from volume_segmantics_amd.data import TrainingDataSlicer
    from volume_segmantics_amd.data.losses import class_weights_from_counts
    from volume_segmantics_amd.model.operations.vol_seg_2d_trainer import resolve_balanced_class_weights
    data, labels = V.volume_pair((6, 7, 8), "uint8_binary", 2)
    slicer = TrainingDataSlicer(data, labels, V.settings())
    assert slicer.num_seg_classes == 2
    with pytest.raises(ValueError, match=KEY) as err:      # the run has three classes, its volumes hold two of them
        resolve_balanced_class_weights(V.settings(**{KEY: "balanced"}), [slicer], 3)
    assert "class 2" in str(err.value)
    with pytest.raises(ValueError, match="no labelled voxel"):
        class_weights_from_counts([5, 0], 2)
    assert class_weights_from_counts([95, 5], 2) == pytest.approx([0.1, 1.9], rel=1e-14)


# ---- the trainer's criteria on the CPU route -----------------------------------------------------------------------------------------
def _trainer(monkeypatch, criterion="DiceLoss", classes=3, **extra):
    from volume_segmantics_amd.model.operations.vol_seg_2d_trainer import VolSeg2dTrainer
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)      # the CPU route, on a GPU host too
    settings = SimpleNamespace(starting_lr=1e-5, end_lr=5.0, lr_find_epochs=1, lr_reduce_factor=500, cuda_device=0, patience=1,
                               loss_criterion=criterion, alpha=0.75, beta=0.25, eval_metric="MeanIoU", pct_lr_inc=0.3, plot_lr_graph=False,
                               image_size=32, training_set_proportion=0.8,
                               model={"type": "U_Net", "encoder_name": "resnet34", "encoder_weights": None}, **extra)
    return VolSeg2dTrainer(None, None, classes, settings, loaders=([], []))


@pytest.mark.parametrize("criterion", ["DiceLoss", "BCEDiceLoss", "BCELoss", "CrossEntropyLoss"])
def test_trainer_criteria_carry_the_weights_on_the_cpu_route(monkeypatch, criterion):
    """the criterion object holds the rescaled weights, and the trainer's own _loss - masked and not - is the float64 formula"""
    from volume_segmantics_amd.data import losses as Lo
    trainer = _trainer(monkeypatch, criterion, **{KEY: [1, 2, 5]})
    want = np.array([3 / 8, 6 / 8, 15 / 8])
    assert trainer.class_weights == pytest.approx(want, rel=1e-15)
    crit = trainer.loss_criterion
    assert isinstance(crit, {"DiceLoss": Lo.DiceLoss, "BCEDiceLoss": Lo.BCEDiceLoss, "BCELoss": nn.BCEWithLogitsLoss,
                             "CrossEntropyLoss": nn.CrossEntropyLoss}[criterion])
    assert np.array_equal(crit.weight.reshape(-1).numpy(), want.astype(np.float32))
    assert isinstance(trainer.eval_metric, Lo.MeanIoU)                      # the metric has no weights
    case = T.Case("small_odd", 3)
    name = "Dice" if criterion == "DiceLoss" else criterion
    for pattern in (None, "random30"):
        logits, onehot, valid = W.case_inputs(case, pattern)
        ref, _grad = W.evaluate(name, logits, onehot, want.astype(np.float32), valid)
        got = trainer._loss(torch.tensor(logits), torch.tensor(onehot), None if valid is None else torch.tensor(valid))
        assert abs(float(got) - ref) <= 2e-6 * max(1.0, abs(ref)), (pattern, float(got), ref)      # float32 torch ops: the project's loss bound


def test_trainer_refusals_and_the_absent_key(monkeypatch):
    from volume_segmantics_amd.data import losses as Lo
    with pytest.raises(ValueError, match="unresolved"):
        _trainer(monkeypatch, **{KEY: "balanced"})
    with pytest.raises(ValueError, match="GeneralizedDiceLoss"):
        _trainer(monkeypatch, "GeneralizedDiceLoss", **{KEY: [1, 1, 1]})
    with pytest.raises(ValueError, match="3 classes"):
        _trainer(monkeypatch, **{KEY: [1, 1]})
    for criterion, kind in (("DiceLoss", Lo.DiceLoss), ("BCEDiceLoss", Lo.BCEDiceLoss), ("BCELoss", nn.BCEWithLogitsLoss),
                            ("CrossEntropyLoss", nn.CrossEntropyLoss), ("GeneralizedDiceLoss", Lo.GeneralizedDiceLoss)):
        trainer = _trainer(monkeypatch, criterion)
        assert trainer.class_weights is None and type(trainer.loss_criterion) is kind
        assert getattr(trainer.loss_criterion, "weight", None) is None and not list(trainer.loss_criterion.state_dict())
    assert Lo.HipDiceLoss().weight is None and Lo.HipSegLoss("BCELoss").weight is None
    assert type(Lo.HipSegLoss("BCELoss").fallback) is nn.BCEWithLogitsLoss and Lo.HipSegLoss("CrossEntropyLoss").fallback.weight is None


# ---- restatements against the reference ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wname", ["ones", "mild", "steep"])
@pytest.mark.parametrize("norm", ["none", "sigmoid"])
def test_weighted_dice_equals_the_reference_projects_numbers(golden, norm, wname):
    """DiceLoss(weight, normalization) of data/losses.py and the formula of class_weight_cases, float64, against the fixture"""
    from volume_segmantics_amd.data.losses import DiceLoss
    g = golden("g11_weighted_losses.npz")
    logits, targets, w = g["logits"], g["targets"], g[f"{wname}__weight"]
    ref_loss, ref_grad = float(g[f"{wname}__{norm}__loss"]), g[f"{wname}__{norm}__grad"]
    assert logits.shape == (2, 3, 9, 7) and logits.dtype == np.float64 and ref_grad.dtype == np.float64
    x = torch.tensor(logits).requires_grad_()
    loss = DiceLoss(weight=torch.tensor(w), normalization=norm)(x, torch.tensor(targets))
    loss.backward()
    assert abs(float(loss.detach()) - ref_loss) <= F64_BOUND and np.abs(x.grad.numpy() - ref_grad).max() <= F64_BOUND * np.abs(ref_grad).max()
    x = torch.tensor(logits).requires_grad_()
    if norm == "none":
        loss = W.weighted_loss("Dice", x, targets, w)
    else:      # the Dice term of the BCE-Dice formula: alpha = 0, beta = 1
        loss = W.weighted_loss("BCEDiceLoss", x, targets, w, alpha=0.0, beta=1.0)
    loss.backward()
    assert abs(float(loss.detach()) - ref_loss) <= F64_BOUND and np.abs(x.grad.numpy() - ref_grad).max() <= F64_BOUND * np.abs(ref_grad).max()


HOST_CASES = (T.Case("small_odd", 2), T.Case("small_odd", 3), T.Case("one_wave", 3), T.Case("small_odd", 3, zero_column=True))


@pytest.mark.parametrize("wset", ["mild", "ratio100"])
@pytest.mark.parametrize("case", HOST_CASES, ids=lambda c: c.id)
def test_weighted_bce_and_cross_entropy_equal_torchs_own_modules(case, wset):
    """nn.BCEWithLogitsLoss(weight = w.view(1, K, 1, 1)) and nn.CrossEntropyLoss(weight = w) in float64, unmasked; the cross entropy also
    with ignore_index against the masked formula"""
    logits, onehot = T.inputs(case)
    w = W.weights(case, wset).astype(np.float64)
    anchors = {"CrossEntropyLoss": lambda x: nn.CrossEntropyLoss(weight=torch.tensor(w))(x, torch.argmax(torch.tensor(onehot), dim=1))}
    if not case.zero_column:
        anchors["BCELoss"] = lambda x: nn.BCEWithLogitsLoss(weight=torch.tensor(w).view(1, -1, 1, 1))(x, torch.tensor(onehot).double())
    for name, anchor in anchors.items():
        x = torch.tensor(logits).double().requires_grad_()
        loss = anchor(x)
        loss.backward()
        ref_loss, ref_grad = W.evaluate(name, logits, onehot, w)
        assert abs(float(loss.detach()) - ref_loss) <= F64_BOUND * max(1.0, abs(ref_loss)), name
        assert np.abs(x.grad.numpy() - ref_grad).max() <= F64_BOUND * np.abs(ref_grad).max(), name
    valid = S.valid_mask(case.base, "random30")
    index = torch.tensor(np.where(valid != 0, onehot.argmax(1), S.IGNORE)).long()
    x = torch.tensor(logits).double().requires_grad_()
    loss = nn.CrossEntropyLoss(weight=torch.tensor(w), ignore_index=S.IGNORE)(x, index)
    loss.backward()
    ref_loss, ref_grad = W.evaluate("CrossEntropyLoss", logits, onehot, w, valid)
    assert abs(float(loss.detach()) - ref_loss) <= F64_BOUND * max(1.0, abs(ref_loss))
    assert np.abs(x.grad.numpy() - ref_grad).max() <= F64_BOUND * np.abs(ref_grad).max()


def _restatement(name, w):
    """the criterion the trainer builds without a GPU, with weights"""
    from volume_segmantics_amd.data import losses as Lo
    wt = torch.tensor(w)
    return {"Dice": lambda: Lo.DiceLoss(weight=wt, normalization="none"), "BCEDiceLoss": lambda: Lo.BCEDiceLoss(T.ALPHA, T.BETA, weight=wt),
            "BCELoss": lambda: nn.BCEWithLogitsLoss(weight=wt.view(1, -1, 1, 1)), "CrossEntropyLoss": lambda: nn.CrossEntropyLoss(weight=wt)}[name]()


@pytest.mark.parametrize("pattern", [None, "random30", "class_absent", "one_pixel"])
@pytest.mark.parametrize("case", HOST_CASES[:3], ids=lambda c: c.id)
def test_weighted_restatements_equal_the_formulas_masked_and_not(case, pattern):
    """data/losses.py in float64 (weights float64 too) against class_weight_cases.weighted_loss; zero gradient under the mask"""
    from volume_segmantics_amd.data import losses as Lo
    logits, onehot, valid = W.case_inputs(case, pattern)
    w = W.weights(case, "ratio100").astype(np.float64)
    for name in W.criteria_of(case):
        crit = _restatement(name, w)
        x = torch.tensor(logits).double().requires_grad_()
        t = torch.tensor(onehot)
        if valid is not None:
            loss = Lo.masked_criterion(crit, x, t, torch.tensor(valid))
        elif name == "CrossEntropyLoss":
            loss = crit(x, torch.argmax(t, dim=1))
        else:
            loss = crit(x, t.double())
        loss.backward()
        ref_loss, ref_grad = W.evaluate(name, logits, onehot, w, valid)
        assert abs(float(loss.detach()) - ref_loss) <= F64_BOUND * max(1.0, abs(ref_loss)), name
        assert np.abs(x.grad.numpy() - ref_grad).max() <= F64_BOUND * max(np.abs(ref_grad).max(), 1e-300), name
        if valid is not None:
            assert not x.grad.numpy()[np.broadcast_to(valid[:, None] == 0, logits.shape)].any(), name
        # the weight handed to masked_criterion itself wins over the criterion's
        if valid is not None and name in ("BCELoss", "CrossEntropyLoss"):
            plain = nn.BCEWithLogitsLoss() if name == "BCELoss" else nn.CrossEntropyLoss()
            again = Lo.masked_criterion(plain, torch.tensor(logits).double(), t, torch.tensor(valid), weight=torch.tensor(w))
            assert abs(float(again) - ref_loss) <= F64_BOUND * max(1.0, abs(ref_loss)), name


def test_no_labelled_pixel_with_weights_gives_the_defined_losses_and_zero_gradients():
    from volume_segmantics_amd.data import losses as Lo
    case = T.Case("small_odd", 3)
    logits, onehot, valid = S.masked_inputs(case, "none")
    poisoned = logits.copy()
    poisoned[0, 0, 0, :3] = (np.nan, np.inf, -np.inf)
    w = W.weights(case, "ratio100")
    for name in W.CRITERIA:
        for x0 in (logits, poisoned):
            x = torch.tensor(x0).requires_grad_()
            loss = Lo.masked_criterion(_restatement(name, w), x, torch.tensor(onehot), torch.tensor(valid))
            loss.backward()
            assert float(loss.detach()) == pytest.approx(S.M0_LOSS[name], abs=1e-7), name
            assert np.isfinite(x.grad.numpy()).all() and not x.grad.numpy().any(), name
            ref, grad = W.evaluate(name, x0, onehot, w, valid)
            assert ref == pytest.approx(S.M0_LOSS[name], abs=1e-12) and not grad.any(), name


def test_module_fallbacks_take_the_weights_on_cpu_tensors():
    """HipDiceLoss / HipSegLoss on CPU tensors go through their torch restatements, with the same weights"""
    from volume_segmantics_amd.data.losses import HipDiceLoss, HipSegLoss
    case = T.Case("small_odd", 3)
    w = W.weights(case, "mild")
    for pattern in (None, "random30"):
        logits, onehot, valid = W.case_inputs(case, pattern)
        for name in W.CRITERIA:
            crit = HipDiceLoss(T.EPS, weight=torch.tensor(w)) if name == "Dice" else HipSegLoss(name, T.ALPHA, T.BETA, T.EPS, weight=torch.tensor(w))
            args = (torch.tensor(logits), torch.tensor(onehot)) + (() if valid is None else (torch.tensor(valid),))
            ref, _grad = W.evaluate(name, logits, onehot, w, valid)
            assert abs(float(crit(*args)) - ref) <= 2e-6 * max(1.0, abs(ref)), (name, pattern)
