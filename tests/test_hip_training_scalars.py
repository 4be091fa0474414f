"""The small kernels at the end of a training step - csrc/loss.hip (default Dice, BCE-Dice, BCE, cross entropy, generalised Dice,
MeanIoU, one-hot) and csrc/optim.hip (AdamW, the per-step scalars) - against the float64 references of tests/training_scalar_cases.py,
at the smallest shapes that reach every launch path: the scalar and the 16-byte Dice kernels, second grid-stride trips, ragged tails,
refused alignments, one to sixteen classes, classes that are absent from the batch, saturated logits.  The cases, the launch each one
selects and the bounds are in that module; tests/test_training_scalars_host.py checks the references and the cases without a GPU."""
import numpy as np
import pytest
import torch

import training_scalar_cases as T

pytestmark = pytest.mark.gpu


def _held(figures, context):
    failed = []
    for label, err, bound in figures:
        print(f"{context} {label}: {err:.3e} of {bound:.3e}")
        if not err <= bound:
            failed.append((label, err, bound))
    assert not failed, (context, failed)


@pytest.mark.parametrize("param", T.LOSS_PARAMS, ids=T.loss_id)
def test_loss_and_gradient_against_float64(param):
    """HipDiceLoss / HipSegLoss with autograd and 1.7 x loss, and the C ABI with a null grad_out into a NaN-filled dlogits:
    |loss - ref| <= 2e-6 max(1, |ref|), max |grad - ref| <= 2e-5 max |ref| with no absolute term (an unwritten element is NaN and
    fails it; where the reference gradient is identically zero the kernel must return zeros)."""
    case, name = param
    _held(T.loss_figures(case, name), f"{case.id} {name}")


@pytest.mark.parametrize("name", T.CRITERIA)
@pytest.mark.parametrize("which", list(T.MISALIGNED))
def test_pointers_off_16_bytes_take_the_scalar_kernels(which, name):
    """2 x 3 x 32 x 32 (hw % 4 == 0) through the C ABI on slices of larger buffers: logits one float in, uint8 targets one byte in,
    float targets or dlogits one float in.  The 16-byte Dice kernels must be refused; the answer meets the same bounds, and the guard
    elements around dlogits stay untouched.  (What this can see is a wrong number: the MI355X carries out a 16-byte access at a
    4-byte-aligned address, so a library that skips the alignment test of vs_dice_loss_bwd gives these numbers too - measured on a
    scratch build.)"""
    tdtype, offsets = T.MISALIGNED[which]
    case = T.Case("misaligned", 3, tdtype=tdtype)
    logits, targets = T.inputs(case)
    ref_loss, ref_grad = T.reference(case, name)
    for grad_out in (None, T.GRAD_OUT):
        loss, grad = T.abi_loss(name, logits, targets, grad_out, offsets)
        _held(T.loss_errors(loss, grad, ref_loss, ref_grad, grad_out or 1.0), f"{which} {name} grad_out={grad_out}")


@pytest.mark.parametrize("tdtype", ["uint8", "float32"])
@pytest.mark.parametrize("classes", T.IOU_CLASSES)
@pytest.mark.parametrize("shape", T.IOU_SHAPES)
def test_mean_iou_against_the_oracle(shape, classes, tdtype):
    """vs_mean_iou on probabilities and on logits (the softmax formed inside the kernel), logits with exact ties and no near-ties"""
    _held(T.iou_figures(shape, classes, tdtype), f"mean_iou {shape} k{classes} {tdtype}")


@pytest.mark.parametrize("classes", T.ONEHOT_CLASSES)
@pytest.mark.parametrize("shape", T.ONEHOT_SHAPES)
def test_onehot_is_bit_equal_to_prepare_training_batch(shape, classes):
    """labels at or above `classes` included: their column stays zero"""
    labels = T.onehot_labels(shape, classes)
    assert (labels >= classes).any() and (labels < classes).any()
    got = T.onehot_device(labels, classes).cpu()
    assert torch.equal(got, T.onehot_reference(labels, classes))


@pytest.mark.parametrize("n", T.ADAMW_SIZES)
def test_adamw_moments_and_update_against_float64(n):
    """vs_adamw_step over the schedule of the case module, each step judged from the device state before it: exp_avg and exp_avg_sq
    within 5e-7 relative, the update p_after - p_before within 8e-6 |update_ref| + 1.5 ulp(p), masked elements bit-identical"""
    failed = []
    for step, figures, changed in T.adamw_run(n):
        for label, ratio in figures:
            print(f"adamw n={n} step {step} {label}: {ratio:.3f} of the bound")
            if not ratio <= 1.0:
                failed.append((step, label, ratio))
        if changed:
            failed.append((step, "masked elements changed", changed))
    assert not failed, failed


def test_adamw_moves_every_unmasked_element():
    """one masked step from non-zero moments: the bits of p, exp_avg and exp_avg_sq change exactly where the mask is set"""
    from volume_segmantics_amd import _lib as L
    n = T.ADAMW_SIZES[1]
    p0, mask, grads = T.adamw_inputs(n)
    g = np.where(grads[0] == 0, np.float32(0.5), grads[0]).astype(np.float32)
    # p with its gradient's sign: decay and update both pull it towards zero and cannot cancel; 0.9 * 0.1 g + 0.1 g and
    # 0.999 * 0.5 g^2 + 0.001 g^2 differ from 0.1 g and 0.5 g^2
    state = [torch.tensor(a).to(T.DEV) for a in (np.copysign(p0, g), 0.1 * g, 0.5 * g * g)]
    before = [a.cpu().numpy().view(np.uint32) for a in state]
    gd, md = torch.tensor(g).to(T.DEV), torch.tensor(mask).to(T.DEV)
    L.check(L.lib.vs_adamw_step(L.ptr(state[0]), L.ptr(gd), L.ptr(state[1]), L.ptr(state[2]), L.ptr(md), n, 1e-2, 0.9, 0.999, 1e-8, 0.01, 4,
                                None))
    torch.cuda.synchronize()
    for a, b in zip(state, before):
        assert np.array_equal(a.cpu().numpy().view(np.uint32) != b, mask != 0)


@pytest.mark.parametrize("hyper", T.HYPER_CASES, ids=lambda h: f"step{h[5]}")
def test_train_hyper_set_writes_the_hosts_float32_scalars(hyper):
    """the eight floats of a recorded step (lr, beta1, beta2, eps, weight decay, 1 - beta1^t, sqrt(1 - beta2^t), t) bit-equal to the
    host's float32 arithmetic; every num_batches_tracked counter up by one, none beside them touched"""
    from volume_segmantics_amd import _lib as L
    lr, b1, b2, eps, wd = (T.f32(v) for v in hyper[:5])
    step = hyper[5]
    out = torch.full((10,), float("nan"), device=T.DEV)
    counters = np.array([0, 1, 2 ** 31 - 1, 2 ** 32 - 1, 2 ** 40] + list(range(100, 170)) + [-7], dtype=np.int64)   # 75 > the 64 threads
    nbt = torch.tensor(counters).to(T.DEV)
    for n_bn in (len(counters) - 1, 0):
        L.check(L.lib.vs_train_hyper_set(L.ptr(out), lr, b1, b2, eps, wd, step, L.ptr(nbt) if n_bn else None, n_bn, None))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got[:8].view(np.uint32), T.host_hyper(lr, b1, b2, eps, wd, step).view(np.uint32)), (got, T.host_hyper(lr, b1, b2, eps, wd, step))
    assert np.isnan(got[8:]).all()
    want = counters.copy()
    want[:-1] += 1
    assert np.array_equal(nbt.cpu().numpy(), want)
