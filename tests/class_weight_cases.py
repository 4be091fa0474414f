"""What the tests of per-class loss weights share (tests/test_class_weights_host.py, tests/test_hip_class_weights.py,
tools/class_weight_probe.py): weight sets, the float64 references, and the device calls of the _weighted entry points of csrc/loss.hip.

The references are the formulas of the feature written out on float64 logits with float64 autograd, w a vector of K weights, every sum
over the labelled pixels (all pixels without a mask), M their count:
    Dice               1 - (1/K) sum_c w_c 2 I_c / clamp(D_c, eps)                    (compute_per_channel_dice(..., weight=w))
    BCELoss            sum_c w_c sum_pix bce(x, t) / (M K)                             (nn.BCEWithLogitsLoss(weight=w.view(1, K, 1, 1)))
    BCEDiceLoss        alpha * the BCE above + beta * the Dice above on sigmoid(x)
    CrossEntropyLoss   sum_pix w_t l / sum_pix w_t, the class the first 1 of the one-hot column (an all-zero column: class 0); 0 when
                       the sum of weights is 0                                          (nn.CrossEntropyLoss(weight=w, ignore_index=...))
No labelled pixel: the BCE and cross-entropy terms are 0, the Dice terms follow their clamped formulas, every gradient is 0.
The host tests anchor these to torch's own modules and to the reference project's DiceLoss(weight=...) (tests/golden/g11_weighted_losses.npz).

The weights reach the kernels as float32 and are used as given; the references take those float32 values, in float64.  Shapes, seeded
inputs, Case and the two bounds (|loss - ref| <= 2e-6 max(1, |ref|), max|grad - ref| <= 2e-5 max|ref|) are those of
training_scalar_cases; the mask patterns those of sparse_label_cases."""
import functools

import numpy as np
import torch

import sparse_label_cases as S
import training_scalar_cases as T

CRITERIA = ("Dice", "BCEDiceLoss", "BCELoss", "CrossEntropyLoss")      # the generalised Dice takes no class weights
WEIGHT_SETS = ("ones", "mild", "balanced", "ratio100")


def criteria_of(case):
    return tuple(c for c in T.criteria_of(case) if c in CRITERIA)


def label_counts(case, pattern=None):
    """labelled pixels per class of the case's one-hot targets (under the mask pattern, if any)"""
    onehot = T.inputs(case.base)[1] if pattern is None else S.masked_inputs(case.base, pattern)[1]
    return onehot.astype(np.int64).sum(axis=(0, 2, 3))


def has_balanced(case, pattern=None):
    return bool((label_counts(case, pattern) > 0).all())


def weights(case, wset, pattern=None):
    """K float32 weights that sum to K (rescaled in float64, then rounded once).  ones: exactly 1.0;  mild: linspace(0.5, 1.5, K);
    balanced: N / (K n_c) from the case's own label counts (a class without a pixel has none: has_balanced);  ratio100: 1 and 100
    alternating - for two classes the pair 1 : 100."""
    k = case.classes
    if wset == "ones":
        raw = np.ones(k)
    elif wset == "mild":
        raw = np.linspace(0.5, 1.5, k)
    elif wset == "balanced":
        counts = label_counts(case, pattern).astype(np.float64)
        assert (counts > 0).all(), "balanced weights need every class among the labelled pixels"
        raw = counts.sum() / (k * counts)
    elif wset == "ratio100":
        raw = np.where(np.arange(k) % 2 == 1, 100.0, 1.0)
    else:
        raise KeyError(wset)
    w = (raw * (k / raw.sum())).astype(np.float32)
    w.setflags(write=False)
    return w


# ---- float64 references ------------------------------------------------------------------------------------------------------------
def weighted_loss(name, x, t, w, valid=None, alpha=T.ALPHA, beta=T.BETA, eps=T.EPS):
    """the formulas of the module docstring: x (n, K, h, w) tensor of any floating dtype, t one-hot, w (K,), valid (n, h, w) or None"""
    k = x.shape[1]
    w = torch.tensor(np.asarray(w)).to(x.dtype)
    keep = torch.ones(x.shape[0], 1, *x.shape[2:], dtype=torch.bool) if valid is None else (torch.tensor(np.asarray(valid)) != 0).unsqueeze(1)
    zero = torch.zeros((), dtype=x.dtype)
    tf = torch.where(keep, torch.tensor(np.asarray(t)).to(x.dtype), zero)
    xs = torch.where(keep, x, zero)
    m = keep.sum()
    wk = w.view(1, k, 1, 1)

    def dice(p):
        p = torch.where(keep, p, zero)
        inter = (p * tf).sum((0, 2, 3))
        denom = (p * p).sum((0, 2, 3)) + (tf * tf).sum((0, 2, 3))
        return 1.0 - (w * 2.0 * inter / denom.clamp(min=eps)).sum() / k

    def bce():
        elem = torch.where(keep, torch.nn.functional.binary_cross_entropy_with_logits(xs, tf, reduction="none") * wk, zero)
        return elem.sum() / (m * k).clamp(min=1)

    if name == "Dice":
        return dice(x)
    if name == "BCELoss":
        return bce()
    if name == "BCEDiceLoss":
        return alpha * bce() + beta * dice(torch.sigmoid(xs))
    if name == "CrossEntropyLoss":
        index = torch.argmax(torch.tensor(np.asarray(t)), dim=1)          # the first maximum: the first 1, or 0 for an all-zero column
        elem = torch.nn.functional.cross_entropy(xs, index, reduction="none")
        wt = torch.where(keep[:, 0], w[index], zero)
        total = wt.sum()
        return (wt * elem).sum() / torch.where(total > 0, total, torch.ones_like(total))
    raise KeyError(name)


def evaluate(name, logits, targets, w, valid=None, dtype=torch.float64):
    """(loss, d loss / d logits for grad_out = 1) of weighted_loss in `dtype`, as float and float64 array"""
    x = torch.tensor(np.asarray(logits)).to(dtype).requires_grad_()
    loss = weighted_loss(name, x, targets, np.asarray(w, dtype=np.float64), valid)
    loss.backward()
    return float(loss.detach().double()), x.grad.double().numpy()


@functools.lru_cache(maxsize=4)
def _reference(case, pattern, wset, name):
    if pattern is None:
        (logits, onehot), valid = T.inputs(case), None
    else:
        logits, onehot, valid = S.masked_inputs(case, pattern)
    loss, grad = evaluate(name, logits, onehot, weights(case, wset, pattern), valid)
    grad.setflags(write=False)
    return loss, grad


def reference(case, pattern, wset, name):
    return _reference(case.base, pattern, wset, name)


def errors(loss, grad, valid, ref_loss, ref_grad, grad_out=1.0):
    """[(label, measured, bound)]: the two bounds of training_scalar_cases, nothing non-finite, and - with a mask - the count of
    ignored elements whose gradient is not the bit pattern of +0.0 (bound 0)"""
    if valid is not None:
        return S.masked_errors(loss, grad, valid, ref_loss, ref_grad, grad_out)
    finite = float(0.0 if np.isfinite(loss) and np.isfinite(grad).all() else np.inf)
    return T.loss_errors(loss, grad, ref_loss, ref_grad, grad_out) + [("non-finite", finite, 0.0)]


# ---- the device side ---------------------------------------------------------------------------------------------------------------
def abi_loss_weighted(name, logits, targets, w, valid=None, grad_out=None):
    """the _weighted entry points straight through the C ABI, valid None: the null mask pointer.  (loss, dlogits) as numpy; dlogits
    lies inside a larger allocation filled with NaN: nothing outside its n k hw elements may be written."""
    from volume_segmantics_amd import _lib as L
    n, k = logits.shape[:2]
    hw = int(np.prod(logits.shape[2:]))
    is_f32 = int(targets.dtype == np.float32)
    x, t = T._offset_copy(logits, 0), T._offset_copy(targets, 0)
    m = None if valid is None else T._offset_copy(valid, 0)
    cw = torch.tensor(np.asarray(w, dtype=np.float32)).to(T.DEV)
    front = 8
    dbuf = torch.full((x.numel() + 2 * front,), float("nan"), dtype=torch.float32, device=T.DEV)
    dx = dbuf[front:front + x.numel()]
    loss = torch.full((), float("nan"), dtype=torch.float32, device=T.DEV)
    g = None if grad_out is None else torch.tensor(float(grad_out), dtype=torch.float32, device=T.DEV)
    if name == "Dice":
        nbytes = L.lib.vs_dice_workspace(k)
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=T.DEV)
        L.check(L.lib.vs_dice_loss_fwd_weighted(L.ptr(x), L.ptr(t), is_f32, L.ptr(m), L.ptr(cw), n, k, hw, T.EPS, L.ptr(loss), L.ptr(ws),
                                                nbytes, None))
        L.check(L.lib.vs_dice_loss_bwd_weighted(L.ptr(x), L.ptr(t), is_f32, L.ptr(m), L.ptr(cw), L.ptr(g), n, k, hw, T.EPS, L.ptr(ws),
                                                L.ptr(dx), None))
    else:
        nbytes = L.lib.vs_seg_loss_weighted_workspace(k)
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=T.DEV)
        L.check(L.lib.vs_seg_loss_fwd_weighted(T.SEG_KINDS[name], L.ptr(x), L.ptr(t), is_f32, L.ptr(m), L.ptr(cw), n, k, hw, T.ALPHA, T.BETA,
                                               T.EPS, L.ptr(loss), L.ptr(ws), nbytes, None))
        L.check(L.lib.vs_seg_loss_bwd_weighted(T.SEG_KINDS[name], L.ptr(x), L.ptr(t), is_f32, L.ptr(m), L.ptr(cw), L.ptr(g), n, k, hw,
                                               L.ptr(ws), L.ptr(dx), None))
    torch.cuda.synchronize()
    guard = torch.cat([dbuf[:front], dbuf[front + x.numel():]])
    assert bool(torch.isnan(guard).all()), "dlogits written outside its n k h w elements"
    return loss.item(), dx.cpu().numpy().reshape(logits.shape)


def module_loss_weighted(name, logits, targets, w, valid=None, grad_out=T.GRAD_OUT):
    """HipDiceLoss / HipSegLoss with weight= (and `valid`) and autograd: (loss, logits.grad) as numpy"""
    from volume_segmantics_amd.data.losses import HipDiceLoss, HipSegLoss
    wt = torch.tensor(np.asarray(w, dtype=np.float32))
    crit = HipDiceLoss(T.EPS, weight=wt) if name == "Dice" else HipSegLoss(name, T.ALPHA, T.BETA, T.EPS, weight=wt)
    x = torch.tensor(np.asarray(logits)).to(T.DEV).requires_grad_()
    t = torch.tensor(np.asarray(targets)).to(T.DEV)
    loss = crit(x, t) if valid is None else crit(x, t, torch.tensor(np.asarray(valid)).to(T.DEV))
    assert loss.is_cuda
    (loss * grad_out).backward()
    torch.cuda.synchronize()
    return loss.item(), x.grad.cpu().numpy()


def case_inputs(case, pattern):
    """(logits, targets, valid or None)"""
    if pattern is None:
        return (*T.inputs(case), None)
    return S.masked_inputs(case, pattern)


def weighted_figures(case, pattern, wset, name):
    """both routes of one (case, mask pattern or None, weight set, criterion): the module with grad_out = 1.7, the C ABI with the null
    grad_out"""
    logits, targets, valid = case_inputs(case, pattern)
    w = weights(case.base, wset, pattern)
    ref_loss, ref_grad = reference(case, pattern, wset, name)
    out = []
    loss, grad = module_loss_weighted(name, logits, targets, w, valid)
    out += [(f"module {label}", err, bound) for label, err, bound in errors(loss, grad, valid, ref_loss, ref_grad, T.GRAD_OUT)]
    loss, grad = abi_loss_weighted(name, logits, targets, w, valid)
    out += [(f"abi {label}", err, bound) for label, err, bound in errors(loss, grad, valid, ref_loss, ref_grad)]
    return out


# The launch each case selects is described in training_scalar_cases.LOSS_CASES; the weights meet
#   small_odd    the scalar kernels, K = 1, 2, 3, 16 (no cross entropy at K = 1), every weight set, with and without a mask
#   one_wave     a single wave
#   stride_odd   the second grid-stride trip of the scalar kernels
#   stride_vec   the 16-byte kernels: vectors crossing sample and class planes, capped grids and their second trips, K = 2 and 5
#   absent/dead  the D <= eps branches (default Dice: logits 0; BCE-Dice: sigmoid = 0), where the clamped term meets a weight
#   zero_column  the cross entropy's all-zero column: class 0's weight
def _params():
    C = T.Case
    rows = []
    for k in (1, 2, 3, 16):
        for wset in WEIGHT_SETS:
            rows += [(C("small_odd", k), None, wset), (C("small_odd", k), "random30", wset)]
    rows += [(C("small_odd", 3, tdtype="float32"), None, "mild"), (C("small_odd", 3, tdtype="float32"), "random30", "mild"),
             (C("one_wave", 3, tdtype="float32"), None, "mild"), (C("one_wave", 1), "random30", "ratio100"),
             (C("stride_odd", 2), None, "balanced"), (C("stride_odd", 3, tdtype="float32"), "rows8", "mild"),
             (C("stride_vec", 2), None, "ratio100"), (C("stride_vec", 2, tdtype="float32"), "rows8", "mild"),
             (C("stride_vec", 5), "rows8", "balanced"), (C("stride_vec", 5, tdtype="float32"), None, "mild")]
    for case in (C("small_odd", 3, absent=0), C("small_odd", 3, absent="last"), C("small_odd", 3, absent="last", dead="zero"),
                 C("small_odd", 3, absent="last", dead="off")):
        rows += [(case, None, "mild"), (case, None, "ratio100")]
    rows += [(C("small_odd", 3), "class_absent", "mild"), (C("small_odd", 3, absent="last", dead="zero"), "random30", "ratio100"),
             (C("small_odd", 3, zero_column=True), None, "mild"), (C("small_odd", 3, zero_column=True, tdtype="float32"), "random30", "ratio100")]
    params =[(case, pattern, wset, name) for case, pattern, wset in rows for name in criteria_of(case)]
    params.sort(key=lambda p: (p[0].shape, p[0].classes, p[0].id, str(p[1]), p[2], CRITERIA.index(p[3])))
    return params


WEIGHTED_PARAMS = _params()


def weighted_id(param):
    case, pattern, wset, name = param
    return f"{case.id}-{pattern or 'unmasked'}-{wset}-{name}"


# bit identity under weights of exactly 1.0: every case of training_scalar_cases on these two shapes, unmasked and under a mask
IDENTITY_PARAMS = [(case, name) for case in T.LOSS_CASES if case.shape in ("small_odd", "stride_vec") for name in criteria_of(case)]
IDENTITY_PATTERN = {"small_odd": "random30", "stride_vec": "rows8"}
