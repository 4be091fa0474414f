"""-m gpu: per-class loss weights on the MI355X - the _weighted entry points of csrc/loss.hip (default Dice, BCE-Dice, BCE, cross
entropy) through HipDiceLoss / HipSegLoss and the C ABI against the float64 formulas of tests/class_weight_cases.py, masked and
unmasked, at the smallest shapes that reach each launch path; bit-equality with the unweighted and _masked entry points under weights
of exactly 1.0; the refusals; one batch through the trainer.

    small_odd (3, 33, 31)       scalar kernels, ragged last workgroup; classes 1, 2, 3, 16; every weight set
    one_wave (1, 5, 7)          a single wave
    stride_odd (1, 363, 363)    second grid-stride trip of the scalar kernels
    stride_vec (5, 660, 640)    K = 2 and 5: the 16-byte kernels, vectors crossing sample and class planes, capped grids, second trips
    absent / dead, K = 3        the D <= eps branches meet a weight;  zero_column: the cross entropy's class-0 weight"""
import logging
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import class_weight_cases as W
import sparse_label_cases as S
import training_scalar_cases as T

pytestmark = pytest.mark.gpu


def _held(figures, context):
    failed = []
    for label, err, bound in figures:
        print(f"{context} {label}: {err:.3e} of {bound:.3e}")
        if not err <= bound:
            failed.append((label, err, bound))
    assert not failed, (context, failed)


@pytest.mark.parametrize("param", W.WEIGHTED_PARAMS, ids=W.weighted_id)
def test_weighted_loss_and_gradient_against_the_float64_formulas(param):
    """HipDiceLoss / HipSegLoss with weight= (autograd, 1.7 x loss) and the C ABI with a null grad_out into a NaN-filled dlogits with
    guard bands: the two bounds of training_scalar_cases; with a mask every ignored element of the gradient is the bit pattern of
    +0.0; nothing is non-finite and nothing inside dlogits stays NaN"""
    case, pattern, wset, name = param
    _held(W.weighted_figures(case, pattern, wset, name), W.weighted_id(param))


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float32).view(np.uint32), np.ascontiguousarray(b, dtype=np.float32).view(np.uint32))


@pytest.mark.parametrize("param", W.IDENTITY_PARAMS, ids=T.loss_id)
def test_weights_of_one_return_the_unweighted_and_the_masked_bits(param):
    """loss and every gradient element: valid null against vs_dice_loss_* / vs_seg_loss_*, with a mask against their _masked forms"""
    case, name = param
    logits, targets = T.inputs(case)
    ones = np.ones(case.classes, np.float32)
    for grad_out in (None, T.GRAD_OUT):
        loss, grad = T.abi_loss(name, logits, targets, grad_out)
        wloss, wgrad = W.abi_loss_weighted(name, logits, targets, ones, None, grad_out)
        assert _same_bits(loss, wloss), (loss, wloss)
        assert _same_bits(grad, wgrad), f"{int((grad.view(np.uint32) != wgrad.view(np.uint32)).sum())} elements differ"
    _x, mtargets, valid = S.masked_inputs(case, W.IDENTITY_PATTERN[case.shape])
    for grad_out in (None, T.GRAD_OUT):
        loss, grad = S.abi_loss_masked(name, logits, mtargets, valid, grad_out)
        wloss, wgrad = W.abi_loss_weighted(name, logits, mtargets, ones, valid, grad_out)
        assert _same_bits(loss, wloss), (loss, wloss)
        assert _same_bits(grad, wgrad), f"{int((grad.view(np.uint32) != wgrad.view(np.uint32)).sum())} elements differ under the mask"


@pytest.mark.parametrize("case", [T.Case("small_odd", 3), T.Case("misaligned", 3, tdtype="float32")], ids=lambda c: c.id)
def test_no_labelled_pixel_with_weights(case):
    """M = 0: BCE and cross-entropy terms 0, Dice terms by their clamped formulas, every gradient +0.0, nothing NaN - with non-finite
    logits under the ignored pixels as well"""
    logits, targets, valid = S.masked_inputs(case, "none")
    poisoned = logits.copy()
    poisoned[0, 0, 0, :3] = (np.nan, np.inf, -np.inf)
    w = W.weights(case, "ratio100")
    for name in W.CRITERIA:
        for x in (logits, poisoned):
            for loss, grad in (W.abi_loss_weighted(name, x, targets, w, valid), W.module_loss_weighted(name, x, targets, w, valid)):
                assert abs(loss - S.M0_LOSS[name]) <= T.LOSS_BOUND, (name, loss)
                assert not np.ascontiguousarray(grad).view(np.uint32).any(), name


def test_refusals_launch_nothing():
    """kind 4 with weights, a null class_weights and a workspace that is too small: VS_ERR_INVALID with a message; loss and dlogits
    keep their NaN fill"""
    from volume_segmantics_amd import _lib as L
    case = T.Case("small_odd", 3)
    logits, targets = T.inputs(case)
    n, k = logits.shape[:2]
    hw = logits.shape[2] * logits.shape[3]
    x, t = torch.tensor(logits).to(T.DEV), torch.tensor(targets).to(T.DEV)
    cw = torch.ones(k, device=T.DEV)
    dx = torch.full_like(x, float("nan"))
    loss = torch.full((), float("nan"), device=T.DEV)
    seg_bytes, dice_bytes = L.lib.vs_seg_loss_weighted_workspace(k), L.lib.vs_dice_workspace(k)
    assert seg_bytes == L.lib.vs_seg_loss_masked_workspace(k) + 64
    ws = torch.zeros(seg_bytes // 4, device=T.DEV)
    p = L.ptr

    def seg_fwd(kind, weights, nbytes):
        return L.lib.vs_seg_loss_fwd_weighted(kind, p(x), p(t), 0, None, p(weights), n, k, hw, T.ALPHA, T.BETA, T.EPS, p(loss), p(ws), nbytes, None)

    def seg_bwd(kind, weights):
        return L.lib.vs_seg_loss_bwd_weighted(kind, p(x), p(t), 0, None, p(weights), None, n, k, hw, p(ws), p(dx), None)

    def dice_fwd(weights, nbytes):
        return L.lib.vs_dice_loss_fwd_weighted(p(x), p(t), 0, None, p(weights), n, k, hw, T.EPS, p(loss), p(ws), nbytes, None)

    def dice_bwd(weights):
        return L.lib.vs_dice_loss_bwd_weighted(p(x), p(t), 0, None, p(weights), None, n, k, hw, T.EPS, p(ws), p(dx), None)

    for call, word in ((lambda: seg_fwd(4, cw, seg_bytes), "generalised"), (lambda: seg_bwd(4, cw), "generalised"),
                       (lambda: seg_fwd(2, None, seg_bytes), "class_weights"), (lambda: seg_bwd(2, None), "class_weights"),
                       (lambda: dice_fwd(None, dice_bytes), "class_weights"), (lambda: dice_bwd(None), "class_weights"),
                       (lambda: seg_fwd(1, cw, seg_bytes - 4), "workspace"), (lambda: seg_fwd(3, cw, L.lib.vs_seg_loss_masked_workspace(k)), "workspace"),
                       (lambda: dice_fwd(cw, dice_bytes - 4), "workspace")):
        assert call() == -1 and word in L.last_error(), L.last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(loss)) and bool(torch.isnan(dx).all())
    assert seg_fwd(2, cw, seg_bytes) == 0 and seg_bwd(2, cw) == 0          # .. and the same arguments, complete, are taken
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(dx).all())


# ---- trainer -----------------------------------------------------------------------------------------------------------------------
def _thin_batches(seed=0, count=4, size=64):
    """2 classes, about 5 % foreground: a smoothed field thresholded at its 95th percentile"""
    rng = np.random.default_rng([9100, seed])
    field = rng.standard_normal((count, size, size)).astype(np.float32)
    for ax in (1, 2):
        for _ in range(2):
            field = (np.roll(field, 1, ax) + field + np.roll(field, -1, ax)) / 3
    masks = (field > np.percentile(field, 95)).astype(np.uint8)
    imgs = np.clip(128 + 300 * field + 40 * masks, 0, 255).astype(np.uint8)
    return imgs, masks


def _trainer(weights=None, step_mode=None):
    from torch.utils.data import DataLoader
    from volume_segmantics_amd.data.datasets import ArraySliceDataset
    from volume_segmantics_amd.model.operations.vol_seg_2d_trainer import VolSeg2dTrainer
    imgs, masks = _thin_batches()
    loaders = (DataLoader(ArraySliceDataset(imgs, masks), batch_size=4), DataLoader(ArraySliceDataset(imgs, masks), batch_size=4))
    settings = SimpleNamespace(starting_lr=1e-4, end_lr=1e-2, lr_find_epochs=1, lr_reduce_factor=500, cuda_device=0, patience=3,
                               loss_criterion="DiceLoss", alpha=0.75, beta=0.25, eval_metric="MeanIoU", pct_lr_inc=0.3, plot_lr_graph=False,
                               image_size=64, training_set_proportion=0.8, precision="fp32",
                               model={"type": "U_Net", "encoder_name": "resnet18", "encoder_weights": None})
    if weights is not None:
        settings.loss_class_weights = weights
    if step_mode is not None:
        settings.step_mode = step_mode
    torch.manual_seed(31)
    trainer = VolSeg2dTrainer(None, None, 2, settings, loaders=loaders)
    trainer._create_model_and_optimiser(1e-3)
    trainer.model.train()
    return trainer, masks


def _one_step(trainer):
    """the trainer's own step on its one batch: (loss bits, gradients, parameters after the update)"""
    scheduler = torch.optim.lr_scheduler.LambdaLR(trainer.optimizer, lambda step: 1.0)
    batch = next(iter(trainer.training_loader))
    loss = trainer._train_one_batch(scheduler, batch).detach()
    torch.cuda.synchronize()
    grads = [p.grad.detach().cpu().numpy().copy() for p in trainer.model.parameters() if p.grad is not None]
    params = [p.detach().cpu().numpy().copy() for p in trainer.model.parameters()]
    return np.float32(loss.item()), grads, params


def test_trainer_batch_with_balanced_weights_equals_the_float64_formula():
    from volume_segmantics_amd.data.losses import HipDiceLoss, class_weights_from_counts
    _probe, masks = _trainer()
    counts = np.bincount(masks.reshape(-1), minlength=2)
    assert 0.03 < counts[1] / counts.sum() < 0.07
    balanced = class_weights_from_counts(counts, 2)
    trainer, _masks = _trainer(weights=balanced)
    assert isinstance(trainer.loss_criterion, HipDiceLoss) and trainer.class_weights == pytest.approx(balanced, rel=1e-12)
    w32 = np.asarray(trainer.class_weights, dtype=np.float32)
    assert np.array_equal(trainer.loss_criterion.weight.cpu().numpy(), w32)
    batch = next(iter(trainer.training_loader))
    with torch.no_grad():
        inputs, targets, valid = trainer._batch(batch)
        output = trainer.model(inputs)
        loss = trainer._loss(output, targets, valid)
    assert valid is None and loss.is_cuda
    ref, _grad = W.evaluate("Dice", output.cpu().numpy(), targets.cpu().numpy(), w32)
    unweighted, _grad = W.evaluate("Dice", output.cpu().numpy(), targets.cpu().numpy(), np.ones(2, np.float32))
    print(f"trainer balanced {w32}: loss {loss.item():.7f}, float64 formula {ref:.7f}, unweighted {unweighted:.7f}")
    assert abs(loss.item() - ref) <= T.LOSS_BOUND * max(1.0, abs(ref))
    assert abs(ref - unweighted) > 100 * T.LOSS_BOUND                      # the weights matter on this batch


def test_trainer_batch_with_unit_weights_is_bit_equal_to_no_key():
    plain = _one_step(_trainer()[0])
    unit_trainer, _masks = _trainer(weights=[1, 1])
    assert unit_trainer.class_weights == [1.0, 1.0]
    unit = _one_step(unit_trainer)
    assert plain[0].view(np.uint32) == unit[0].view(np.uint32), (plain[0], unit[0])
    assert len(plain[1]) == len(unit[1]) > 0 and len(plain[2]) == len(unit[2])
    for a, b in zip(plain[1] + plain[2], unit[1] + unit[2]):
        assert _same_bits(a, b)


def test_graph_step_mode_with_weights_runs_call_by_call_and_says_so_once(caplog):
    trainer, _masks = _trainer(weights=[1, 3], step_mode="graph")
    scheduler = torch.optim.lr_scheduler.LambdaLR(trainer.optimizer, lambda step: 1.0)
    batch = next(iter(trainer.training_loader))
    with caplog.at_level(logging.INFO):
        losses = [float(trainer._train_one_batch(scheduler, batch)) for _ in range(3)]
    assert np.isfinite(losses).all()
    lines = [r.getMessage() for r in caplog.records if "call by call" in r.getMessage()]
    assert len(lines) == 1 and "loss_class_weights" in lines[0]
