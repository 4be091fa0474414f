"""What the tests of training on partly labelled volumes share (tests/test_sparse_labels_host.py, tests/test_hip_sparse_labels.py,
tools/sparse_label_probe.py): mask patterns, the compaction oracle, and the device calls of the masked entry points of csrc/loss.hip.

The oracle is compaction.  Every criterion is a function of sums over pixels, so the masked loss on (n, K, h, w) equals the float64
reference of tests/training_scalar_cases.py - unchanged, and unaware of masks - evaluated on the (1, K, 1, M) tensors that hold only the
valid pixels; the masked gradient is that reference's gradient scattered back, 0 elsewhere.  MeanIoU is compacted per sample and the
samples without a valid pixel are left out.  The one thing compaction cannot state is the batch with no valid pixel (a mean over
nothing): there the rule of the feature is written out in M0_LOSS - BCE and cross-entropy terms 0, Dice terms 1 by their clamped
formulas, every gradient 0.  Shapes, seeded inputs and the bounds are those of training_scalar_cases."""
import functools

import numpy as np
import torch

import training_scalar_cases as T

IGNORE = 255
PATTERNS = ("random30", "rows8", "sample_out", "one_pixel", "none", "class_absent")
EXTRA_PATTERNS = ("foreground_only",)      # one-channel cases: strokes painted on the object alone
M0_LOSS = {"Dice": 1.0, "BCEDiceLoss": T.BETA, "BCELoss": 0.0, "CrossEntropyLoss": 0.0, "GeneralizedDiceLoss": 1.0}


@functools.lru_cache(maxsize=None)
def valid_mask(case, pattern):
    """uint8 (n, h, w), 1 = labelled.  random30: about 30 % valid; rows8: every 8th row (the real workload: a few painted slices or
    rows); sample_out: the whole of sample 0 ignored (with one sample: none valid); one_pixel: exactly one valid pixel in the batch;
    none: no valid pixel; class_absent: every pixel of one class ignored - the last class, or the foreground of a one-channel case -
    so that class is absent among the valid pixels (D <= eps, w = 1 / eps, `live` false); foreground_only (one channel): the
    foreground pixels of every 2nd row and nothing else, so the background is absent among the valid pixels - the complementary
    channel's w = 1 / eps, where the foreground gradient of the generalised Dice is the small difference of large terms."""
    n, h, w = case.nhw
    rng = np.random.default_rng([5000 + n, h, w, case.classes, (PATTERNS + EXTRA_PATTERNS).index(pattern)])
    m = np.zeros((n, h, w), np.uint8)
    if pattern == "random30":
        m[:] = rng.random((n, h, w)) < 0.3
    elif pattern == "rows8":
        m[:, ::8] = 1
    elif pattern == "sample_out":
        m[1:] = 1
    elif pattern == "one_pixel":
        m[n - 1, h // 2, w // 3] = 1
    elif pattern == "class_absent":
        onehot = T.inputs(case.base)[1]
        m[:] = onehot[:, case.classes - 1] == 0 if case.classes > 1 else onehot[:, 0] == 0
    elif pattern == "foreground_only":
        m[:, ::2] = T.inputs(case.base)[1][:, 0, ::2] != 0
    elif pattern != "none":
        raise KeyError(pattern)
    m.setflags(write=False)
    return m


def masked_inputs(case, pattern):
    """(logits, targets, valid): the case's inputs with the one-hot column of every ignored pixel zeroed, as the one-hot kernel writes
    it for the label 255"""
    logits, targets = T.inputs(case)
    valid = valid_mask(case.base, pattern)
    return logits, targets * valid[:, None].astype(targets.dtype), valid


def compact(array, valid):
    """(n, K, h, w) -> (1, K, 1, M): the valid pixels, in sample-major order"""
    n, k = array.shape[:2]
    keep = valid.reshape(-1) != 0
    return np.ascontiguousarray(array.reshape(n, k, -1).transpose(1, 0, 2).reshape(k, -1)[:, keep]).reshape(1, k, 1, -1)


def scatter(grad, valid, shape):
    """the inverse of compact for a gradient: 0 at ignored pixels"""
    n, k = shape[:2]
    keep = valid.reshape(-1) != 0
    flat = np.zeros((k, keep.size), np.float64)
    flat[:, keep] = grad.reshape(k, -1)
    return np.ascontiguousarray(flat.reshape(k, n, -1).transpose(1, 0, 2)).reshape(shape)


def oracle(name, logits, onehot, valid):
    """float64 (loss, gradient for grad_out = 1) of the masked criterion, by compaction"""
    if not valid.any():
        return M0_LOSS[name], np.zeros(logits.shape, np.float64)
    loss, grad = T.evaluate(name, compact(logits, valid), compact(onehot, valid), torch.float64)
    return loss, scatter(grad, valid, logits.shape)


@functools.lru_cache(maxsize=4)
def _reference(case, pattern, name):
    logits, onehot, valid = masked_inputs(case, pattern)
    loss, grad = oracle(name, logits, onehot, valid)
    grad.setflags(write=False)
    return loss, grad


def reference(case, pattern, name):
    return _reference(case.base, pattern, name)


def masked_errors(loss, grad, valid, ref_loss, ref_grad, grad_out=1.0):
    """[(label, measured, bound)]: the two bounds of training_scalar_cases, and the count of ignored elements whose gradient is not
    the bit pattern of +0.0 (bound 0).  Where the reference gradient is identically zero the bound is zero: the kernel returns zeros."""
    ignored = np.broadcast_to(valid[:, None] == 0, grad.shape)
    nonzero_bits = int((np.ascontiguousarray(grad, dtype=np.float32).view(np.uint32)[ignored] != 0).sum())
    finite = float(0.0 if np.isfinite(loss) and np.isfinite(grad).all() else np.inf)
    return T.loss_errors(loss, grad, ref_loss, ref_grad, grad_out) + [("bits set at ignored pixels", nonzero_bits, 0), ("non-finite", finite, 0.0)]


# ---- the device side ---------------------------------------------------------------------------------------------------------------
def abi_loss_masked(name, logits, targets, valid, grad_out=None, valid_offset=0):
    """T.abi_loss for the _masked entry points; valid_offset: bytes by which the mask pointer is moved off its allocation"""
    from volume_segmantics_amd import _lib as L
    n, k = logits.shape[:2]
    hw = int(np.prod(logits.shape[2:]))
    is_f32 = int(targets.dtype == np.float32)
    x, t, m = T._offset_copy(logits, 0), T._offset_copy(targets, 0), T._offset_copy(valid, valid_offset)
    dbuf = torch.full((x.numel() + 8,), float("nan"), dtype=torch.float32, device=T.DEV)
    dx = dbuf[:x.numel()]
    loss = torch.full((), float("nan"), dtype=torch.float32, device=T.DEV)
    g = None if grad_out is None else torch.tensor(float(grad_out), dtype=torch.float32, device=T.DEV)
    if name == "Dice":
        nbytes = L.lib.vs_dice_workspace(k)
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=T.DEV)
        L.check(L.lib.vs_dice_loss_fwd_masked(L.ptr(x), L.ptr(t), is_f32, L.ptr(m), n, k, hw, T.EPS, L.ptr(loss), L.ptr(ws), nbytes, None))
        L.check(L.lib.vs_dice_loss_bwd_masked(L.ptr(x), L.ptr(t), is_f32, L.ptr(m), L.ptr(g), n, k, hw, T.EPS, L.ptr(ws), L.ptr(dx), None))
    else:
        nbytes = L.lib.vs_seg_loss_masked_workspace(k)
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=T.DEV)
        L.check(L.lib.vs_seg_loss_fwd_masked(T.SEG_KINDS[name], L.ptr(x), L.ptr(t), is_f32, L.ptr(m), n, k, hw, T.ALPHA, T.BETA, T.EPS,
                                             L.ptr(loss), L.ptr(ws), nbytes, None))
        L.check(L.lib.vs_seg_loss_bwd_masked(T.SEG_KINDS[name], L.ptr(x), L.ptr(t), is_f32, L.ptr(m), L.ptr(g), n, k, hw, L.ptr(ws),
                                             L.ptr(dx), None))
    torch.cuda.synchronize()
    assert bool(torch.isnan(dbuf[x.numel():]).all()), "dlogits written outside its n k h w elements"
    return loss.item(), dx.cpu().numpy().reshape(logits.shape)


def module_loss_masked(name, logits, targets, valid, grad_out=T.GRAD_OUT):
    """HipDiceLoss / HipSegLoss with `valid` and autograd: (loss, logits.grad) as numpy"""
    from volume_segmantics_amd.data.losses import HipDiceLoss, HipSegLoss
    crit = HipDiceLoss(T.EPS) if name == "Dice" else HipSegLoss(name, T.ALPHA, T.BETA, T.EPS)
    x = torch.tensor(np.asarray(logits)).to(T.DEV).requires_grad_()
    loss = crit(x, torch.tensor(np.asarray(targets)).to(T.DEV), torch.tensor(np.asarray(valid)).to(T.DEV))
    assert loss.is_cuda
    (loss * grad_out).backward()
    torch.cuda.synchronize()
    return loss.item(), x.grad.cpu().numpy()


def masked_figures(case, pattern, name, valid_offset=0):
    """both routes of one (case, pattern, criterion): the module with grad_out = 1.7, the C ABI with the null grad_out"""
    logits, targets, valid = masked_inputs(case, pattern)
    ref_loss, ref_grad = reference(case, pattern, name)
    out = []
    if not valid_offset:
        loss, grad = module_loss_masked(name, logits, targets, valid)
        out += [(f"module {label}", err, bound) for label, err, bound in masked_errors(loss, grad, valid, ref_loss, ref_grad, T.GRAD_OUT)]
    loss, grad = abi_loss_masked(name, logits, targets, valid, None, valid_offset)
    out += [(f"abi {label}", err, bound) for label, err, bound in masked_errors(loss, grad, valid, ref_loss, ref_grad)]
    return out


# ---- torch restatements (the CPU route) ----------------------------------------------------------------------------------------------
def restatement(name):
    """f(logits, one-hot targets, valid) -> scalar: the criterion the trainer builds without a GPU, with the mask"""
    from torch import nn
    from volume_segmantics_amd.data import losses as Lo
    crit = {"Dice": lambda: Lo.DiceLoss(normalization="none"), "BCEDiceLoss": lambda: Lo.BCEDiceLoss(T.ALPHA, T.BETA),
            "BCELoss": nn.BCEWithLogitsLoss, "CrossEntropyLoss": nn.CrossEntropyLoss,
            "GeneralizedDiceLoss": lambda: Lo.GeneralizedDiceLoss(epsilon=T.EPS)}[name]()
    return lambda x, t, valid: Lo.masked_criterion(crit, x, t, valid)


def restatement_evaluate(name, logits, targets, valid, dtype=torch.float64):
    x = torch.tensor(np.asarray(logits)).to(dtype).requires_grad_()
    loss = restatement(name)(x, torch.tensor(np.asarray(targets)), torch.tensor(np.asarray(valid)))
    loss.backward()
    return float(loss.detach().double()), x.grad.double().numpy()


# ---- MeanIoU ---------------------------------------------------------------------------------------------------------------------
def iou_reference(probs, onehot, valid):
    """oracle.predictor_numpy.mean_iou per sample on its valid pixels; samples without one left out; NaN when none is left"""
    from oracle import predictor_numpy as P
    scores = []
    for b in range(probs.shape[0]):
        keep = torch.as_tensor(np.asarray(valid[b]).reshape(-1) != 0)
        if bool(keep.any()):
            c = probs.shape[1]
            scores.append(float(P.mean_iou(probs[b].reshape(1, c, -1)[:, :, keep].unsqueeze(2), onehot[b].reshape(1, c, -1)[:, :, keep].unsqueeze(2))))
    return float(np.mean(scores)) if scores else float("nan")


# ---- slicer volumes ----------------------------------------------------------------------------------------------------------------
SPARSE_SHAPE = (12, 10, 8)


def sparse_volume(ignore=IGNORE, classes=(0, 1, 2), dtype=np.uint8, seed=0):
    """(data, labels) of shape 12 x 10 x 8: labels are `ignore` except z-slices 3 and 7, fully labelled, and the row y = 4 of z-slice
    9, partly labelled (x < 5).  Every class occurs."""
    rng = np.random.default_rng([6000, seed])
    data = rng.integers(0, 256, size=SPARSE_SHAPE, dtype=np.uint8)
    drawn = np.asarray(classes)[rng.integers(0, len(classes), size=SPARSE_SHAPE)]
    labels = np.full(SPARSE_SHAPE, ignore, dtype=np.int64)
    labels[3], labels[7] = drawn[3], drawn[7]
    labels[9, 4, :5] = drawn[9, 4, :5]
    labels[3, 0, :len(classes)] = classes
    return data, labels.astype(dtype)


def kept_slices(labels, ignore):
    """{axis: sorted indices of the slices that hold a labelled voxel}, straight from the definition"""
    lab = np.asarray(labels) != ignore
    return {"z": [i for i in range(lab.shape[0]) if lab[i].any()], "y": [i for i in range(lab.shape[1]) if lab[:, i].any()],
            "x": [i for i in range(lab.shape[2]) if lab[:, :, i].any()]}


# ---- augmentation draws that take every branch -------------------------------------------------------------------------------------
def augment_param_sets(size):
    """one explicit draw (data/augmentations.sample_params' dictionary) per branch of the pipeline that moves mask pixels"""
    base = dict(size=size, crop=None, flip_v=False, rot_k=0, transpose=False, distort=None, clahe_clip=None, intensity=None)
    rng = np.random.default_rng(7000)
    return {
        "identity": dict(base),
        "crop": dict(base, crop=(size // 2 + 3, size // 2 + 3, 0.37, 0.81)),
        "flip": dict(base, flip_v=True),
        "rot1": dict(base, rot_k=1), "rot2": dict(base, rot_k=2), "rot3": dict(base, rot_k=3),
        "transpose": dict(base, transpose=True),
        "elastic": dict(base, distort=("elastic", rng.uniform(-4.8, 4.8, size=(3, 2)).astype(np.float32), 12345)),
        "grid": dict(base, distort=("grid", 1 + rng.uniform(-0.3, 0.3, size=6), 1 + rng.uniform(-0.3, 0.3, size=6))),
        "optical": dict(base, distort=("optical", 0.8, 0, -1)),
        "all": dict(base, crop=(size // 2, size // 2, 0.9, 0.1), flip_v=True, rot_k=3, transpose=True,
                    distort=("optical", -0.9, 1, 0), clahe_clip=2.5, intensity=("gamma", 0.9)),
    }


def sparse_mask_image(size, seed=0):
    """(image, mask) uint8 (size, size): blobs of 0 and 1 with about half the pixels 255, in blocks and as single pixels"""
    rng = np.random.default_rng([8000, size, seed])
    image = rng.integers(0, 256, (size, size), dtype=np.uint8)
    mask = rng.integers(0, 2, (size, size)).astype(np.uint8)
    mask[rng.random((size, size)) < 0.3] = IGNORE
    mask[: size // 4] = IGNORE
    mask[:, -3:] = IGNORE
    return image, mask
