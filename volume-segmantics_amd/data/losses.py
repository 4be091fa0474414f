"""Losses and metrics the trainer can select (reference: volume_segmantics/data/pytorch3dunet_losses.py:15-184 and
pytorch3dunet_metrics.py:16-106, themselves vendored from pytorch-3dunet).  Restated on (N, C, H, W) tensors; torch
ops on the logits the engine returns - SURVEY.md section 8f row N3 lists their fusion as a next step."""
from __future__ import annotations

import logging
import math

import numpy as np
import torch
from torch import nn


def _per_channel(t: torch.Tensor) -> torch.Tensor:
    """(N, C, ...) -> (C, N * ...)"""
    return t.transpose(0, 1).reshape(t.size(1), -1)


# ---- sparse labels ---------------------------------------------------------------------------------------------------------------
# ``valid`` (N, H, W) or (N, H*W), uint8 or bool: 1 where the pixel carries a label (the settings key ``ignore_label``).  Every
# criterion is a function of sums over pixels; with a mask m each sum runs over the valid pixels only, M = sum m replaces the pixel
# count, and an ignored pixel has a gradient of exactly 0.  No pixel valid (M = 0): the BCE and cross-entropy terms are 0, the Dice
# terms follow their formulas (every denominator is clamped: loss 1) - on purpose not torch's NaN, which would stay in AdamW's
# moments for good.  Values are selected (torch.where), not multiplied, and the logits of ignored pixels are replaced by 0 before
# any function of them is formed, so a non-finite logit under an ignored pixel stays out of the sums and of the gradients.
def _mask_like(valid, ref):
    """valid as a bool tensor that broadcasts against ref (N, C, ...)"""
    return (valid.reshape(valid.shape[0], 1, -1) != 0).reshape((ref.shape[0], 1) + tuple(ref.shape[2:]))


def _keep(t, mask):
    return torch.where(mask, t, torch.zeros((), dtype=t.dtype, device=t.device))


def _per_class(weight, ref):
    """K class weights in ref's dtype, shaped to broadcast against ref (N, K, ...)"""
    return weight.reshape(-1).to(device=ref.device, dtype=ref.dtype).reshape((1, -1) + (1,) * (ref.dim() - 2))


def masked_bce_with_logits(input, target, valid, weight=None):
    """BCEWithLogitsLoss over the valid pixels: sum / (M K); 0 when M = 0.  ``weight``: K class weights, the element of class c is
    multiplied by w_c (nn.BCEWithLogitsLoss(weight=w.view(1, K, 1, 1)))."""
    mask = _mask_like(valid, input)
    elem = nn.functional.binary_cross_entropy_with_logits(_keep(input, mask), target.to(input.dtype), reduction="none")
    if weight is not None:
        elem = elem * _per_class(weight, input)
    return _keep(elem, mask).sum() / (mask.sum() * input.size(1)).clamp(min=1)


def masked_cross_entropy(input, target, valid, weight=None):
    """CrossEntropyLoss over the valid pixels, the class index the arg-max of the one-hot target: sum / M - what
    nn.CrossEntropyLoss(ignore_index=...) computes - and 0 when M = 0.  ``weight``: K class weights, sum w_t l / sum w_t over the
    valid pixels (nn.CrossEntropyLoss(weight=w, ignore_index=...)), and 0 when that sum of weights is 0."""
    mask = _mask_like(valid, input)
    index = torch.argmax(target, dim=1)
    elem = nn.functional.cross_entropy(_keep(input, mask), index, reduction="none").unsqueeze(1)
    if weight is not None:
        w = _keep(weight.reshape(-1).to(device=input.device, dtype=input.dtype)[index].unsqueeze(1), mask)
        total = w.sum()
        return (w * _keep(elem, mask)).sum() / torch.where(total > 0, total, torch.ones_like(total))
    return _keep(elem, mask).sum() / mask.sum().clamp(min=1)


def weighted_bce_with_logits(input, target, weight):
    """nn.BCEWithLogitsLoss(weight=w.view(1, K, 1, 1)) for any number of trailing dimensions: sum_c w_c sum bce / (N K H W)"""
    return nn.functional.binary_cross_entropy_with_logits(input, target.to(input.dtype), weight=_per_class(weight, input))


# ---- per-class loss weights --------------------------------------------------------------------------------------------------------
# The settings key ``loss_class_weights``: a list of K numbers (one per relabelled class 0 .. K-1, ascending label value) or
# ``balanced``.  The weights enter as the reference's ``weight=`` arguments do (pytorch3dunet_losses.py:15-41, 94-135, 317-339):
#   DiceLoss      1 - (1/K) sum_c w_c 2 I_c / clamp(D_c)             BCELoss           sum_c w_c sum_pix bce / (M K)
#   BCEDiceLoss   alpha weighted BCE + beta weighted Dice(sigmoid)    CrossEntropyLoss  sum_pix w_t l / sum_pix w_t
# and are rescaled to sum to K, so that with mean weight 1 the loss keeps the scale the learning-rate settings were chosen for.
CLASS_WEIGHTS_KEY = "loss_class_weights"


def _rescaled(values, num_classes):
    w = np.asarray(values, dtype=np.float64)
    return [float(v) for v in w * (num_classes / w.sum())]


def class_weights_from_counts(counts, num_classes):
    """``balanced``: w_c = N / (K n_c) from the labelled voxels n_c per class (N = sum n_c), rescaled to sum to K"""
    counts = np.asarray(counts, dtype=np.float64).reshape(-1)
    if counts.size != num_classes:
        raise ValueError(f"{CLASS_WEIGHTS_KEY}: balanced: {counts.size} class counts for {num_classes} classes")
    if (counts <= 0).any():
        raise ValueError(f"{CLASS_WEIGHTS_KEY}: balanced: class {int(np.argmin(counts))} has no labelled voxel in the label volumes "
                         f"of this run (counts {[int(c) for c in counts]})")
    return _rescaled(counts.sum() / (num_classes * counts), num_classes)


def resolve_class_weights(spec, num_classes, criterion=None):
    """The value of ``loss_class_weights`` as the K float64 weights the criteria use (sum K), or None when the key is absent.
    Anything but a list of K finite numbers > 0 is a ValueError - ``balanced`` too: the label counts it needs are with the slicers
    (VolSeg2dTrainer.from_volumes and the train command put the list in its place)."""
    if spec is None:
        return None
    key = CLASS_WEIGHTS_KEY
    if isinstance(spec, str):
        if spec.strip().lower() == "balanced":
            raise ValueError(f"{key}: balanced is unresolved: it is computed from the label volumes, by VolSeg2dTrainer.from_volumes "
                             f"or the train command (resolve_balanced_class_weights), before the trainer is built")
        raise ValueError(f"{key}: '{spec}' is not valid: a list of {num_classes} numbers (one per class) or 'balanced'")
    if criterion == "GeneralizedDiceLoss":
        raise ValueError(f"{key}: GeneralizedDiceLoss has its own inverse-volume class weights and takes none")
    try:
        given = [float(v) for v in spec]
    except (TypeError, ValueError):
        raise ValueError(f"{key}: {spec!r} is not valid: a list of {num_classes} numbers (one per class) or 'balanced'") from None
    if len(given) != num_classes:
        raise ValueError(f"{key}: {len(given)} weights for {num_classes} classes: the list has one entry per class")
    for c, v in enumerate(given):
        if not math.isfinite(v) or v <= 0:
            raise ValueError(f"{key}: the weight of class {c} is {v}: every weight must be finite and > 0")
    used = _rescaled(given, num_classes)
    logging.info(f"{key}: given {given}, used (rescaled to sum to {num_classes}) {used}")
    return used


def class_weight_tensor(weight, device=None):
    """weights as the float32 tensor the criteria keep (None stays None)"""
    if weight is None:
        return None
    return torch.as_tensor(weight, dtype=torch.float64).to(dtype=torch.float32, device=device).reshape(-1)


def compute_per_channel_dice(input, target, epsilon=1e-6, weight=None, valid=None):
    """2 * sum(x t) / clamp(sum(x^2) + sum(t^2)) per channel (V-Net form, pytorch3dunet_losses.py:15-41)."""
    if input.size() != target.size():
        raise ValueError("'input' and 'target' must have the same shape")
    if valid is not None:
        mask = _mask_like(valid, input)
        input, target = _keep(input, mask), _keep(target.float(), mask)
    x, t = _per_channel(input), _per_channel(target).float()
    inter = (x * t).sum(-1)
    if weight is not None:
        inter = weight * inter
    denom = (x * x).sum(-1) + (t * t).sum(-1)
    return 2 * (inter / denom.clamp(min=epsilon))


class DiceLoss(nn.Module):
    """1 - mean per-channel Dice; ``normalization`` in {'sigmoid', 'softmax', 'none'} (the trainer uses 'none',
    vol_seg_2d_trainer.py:133-135, i.e. the loss acts on raw logits)."""

    def __init__(self, weight=None, normalization="sigmoid"):
        super().__init__()
        if normalization not in ("sigmoid", "softmax", "none"):
            raise ValueError(normalization)
        self.register_buffer("weight", weight)
        self.normalization = {"sigmoid": torch.sigmoid, "softmax": lambda x: torch.softmax(x, 1), "none": lambda x: x}[normalization]

    def forward(self, input, target, valid=None):
        if valid is not None:
            input = _keep(input, _mask_like(valid, input))
        return 1.0 - torch.mean(compute_per_channel_dice(self.normalization(input), target, weight=self.weight, valid=valid))


def _valid_u8(valid, n, hw):
    """the mask as the kernels read it: contiguous uint8, n * hw elements"""
    if valid.dtype != torch.uint8:
        valid = (valid != 0).to(torch.uint8)
    valid = valid.contiguous()
    if valid.numel() != n * hw:
        raise ValueError(f"valid has {valid.numel()} elements for {n} samples of {hw} pixels")
    return valid


def _on_device(module, device):
    """the module's class-weight buffer on ``device``: moved once, then kept there"""
    if module.weight.device != device:
        module.weight = module.weight.to(device)
    return module.weight


class _FusedDiceFn(torch.autograd.Function):
    """DiceLoss(normalization="none") forward + gradient as two HIP sweeps (vs_dice_loss_fwd / _bwd; with ``valid`` their _masked
    forms, which leave the same per-class sums in the workspace; with ``weight`` - K float32 class weights on the device - the
    _weighted forms, masked or not)."""

    @staticmethod
    def forward(ctx, logits, targets, eps, group=None, valid=None, weight=None):
        from .. import _lib
        n, k = logits.shape[:2]
        hw = logits[0, 0].numel()
        logits = logits.contiguous()
        targets = targets.contiguous()
        is_f32 = targets.dtype == torch.float32
        if not is_f32 and targets.dtype != torch.uint8:
            targets, is_f32 = targets.float(), True
        ws = torch.empty(_lib.lib.vs_dice_workspace(k) // 4, dtype=torch.float32, device=logits.device)
        loss = torch.empty((), dtype=torch.float32, device=logits.device)
        if weight is not None:
            if weight.numel() != k:
                raise ValueError(f"{weight.numel()} class weights for {k} classes")
            valid = None if valid is None else _valid_u8(valid, n, hw)
            _lib.check(_lib.lib.vs_dice_loss_fwd_weighted(_lib.ptr(logits), _lib.ptr(targets), int(is_f32), _lib.ptr(valid), _lib.ptr(weight),
                                                         n, k, hw, eps, _lib.ptr(loss), _lib.ptr(ws), ws.numel() * 4, _lib.stream_ptr()))
        elif valid is None:
            _lib.check(_lib.lib.vs_dice_loss_fwd(_lib.ptr(logits), _lib.ptr(targets), int(is_f32), n, k, hw, eps, _lib.ptr(loss),
                                                _lib.ptr(ws), ws.numel() * 4, _lib.stream_ptr()))
        else:
            valid = _valid_u8(valid, n, hw)
            _lib.check(_lib.lib.vs_dice_loss_fwd_masked(_lib.ptr(logits), _lib.ptr(targets), int(is_f32), _lib.ptr(valid), n, k, hw, eps,
                                                       _lib.ptr(loss), _lib.ptr(ws), ws.numel() * 4, _lib.stream_ptr()))
        world = 1
        if group is not None:
            import torch.distributed as dist
            world = dist.get_world_size(group)
        if world > 1:
            # the Dice of the GLOBAL batch (the reference's single loader sees all of it): the per-class sums I_c, D_c - the last 2 k
            # floats of the workspace, which the gradient sweep reads - summed over the ranks; the loss from the global sums
            stats = ws[ws.numel() - 2 * k:]
            dist.all_reduce(stats, group=group)
            inter, denom = stats.view(k, 2)[:, 0].double(), stats.view(k, 2)[:, 1].double()
            dice = 2.0 * inter / denom.clamp(min=eps)
            loss = (1.0 - (dice if weight is None else weight.double() * dice).mean()).float()
        ctx.save_for_backward(logits, targets, ws, *(() if valid is None else (valid,)))
        ctx.class_weight = weight
        ctx.meta = (n, k, hw, eps, is_f32, world)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        from .. import _lib
        logits, targets, ws, *valid = ctx.saved_tensors
        n, k, hw, eps, is_f32, world = ctx.meta
        dx = torch.empty_like(logits)
        # (global Dice: every rank holds d loss / d its own logits; the gradient all-reduce AVERAGES the ranks' parameter gradients,
        # the global loss wants their SUM)
        g = (grad_out if world == 1 else grad_out * float(world)).contiguous().float()    # (one rank: no multiply launch)
        if ctx.class_weight is not None:
            _lib.check(_lib.lib.vs_dice_loss_bwd_weighted(_lib.ptr(logits), _lib.ptr(targets), int(is_f32), _lib.ptr(valid[0] if valid else None),
                                                         _lib.ptr(ctx.class_weight), _lib.ptr(g), n, k, hw, eps, _lib.ptr(ws), _lib.ptr(dx),
                                                         _lib.stream_ptr()))
        elif not valid:
            _lib.check(_lib.lib.vs_dice_loss_bwd(_lib.ptr(logits), _lib.ptr(targets), int(is_f32), _lib.ptr(g), n, k, hw, eps,
                                                _lib.ptr(ws), _lib.ptr(dx), _lib.stream_ptr()))
        else:
            _lib.check(_lib.lib.vs_dice_loss_bwd_masked(_lib.ptr(logits), _lib.ptr(targets), int(is_f32), _lib.ptr(valid[0]), _lib.ptr(g),
                                                       n, k, hw, eps, _lib.ptr(ws), _lib.ptr(dx), _lib.stream_ptr()))
        return dx, None, None, None, None, None


class HipDiceLoss(nn.Module):
    """Drop-in for DiceLoss(normalization="none") on GPU tensors (falls through to the torch ops for anything else,
    e.g. CPU tensors in the tests of the host logic).  ``weight``: K class weights, used as given (kept as a float32 buffer; both
    routes take them).  ``global_group``: a torch.distributed group - the loss is
    then the Dice of the GLOBAL batch (per-class sums all-reduced; with SyncBatchNorm, N ranks train exactly the step one process
    would run on the whole batch); default: every rank's own batch, as under a DistributedDataParallel wrap of the reference."""

    def __init__(self, epsilon: float = 1e-6, global_group=None, weight=None):
        super().__init__()
        self.epsilon = epsilon
        self.global_group = global_group
        self.register_buffer("weight", class_weight_tensor(weight))
        self._torch = DiceLoss(weight=class_weight_tensor(weight), normalization="none")

    def forward(self, input, target, valid=None):
        if input.is_cuda and input.dtype == torch.float32 and input.dim() >= 3 and input.shape == target.shape:
            # the cross-rank Dice is a TRAINING construct (it pairs with SyncBatchNorm's global batch): under torch.no_grad() - the
            # validation loop - every rank evaluates its own batches, whose count can differ between ranks when the last global
            # batch is partial (a rank with an empty share skips it), so a collective there would be mismatched across ranks
            group = self.global_group if (torch.is_grad_enabled() and input.requires_grad) else None
            if self.weight is not None:
                return _FusedDiceFn.apply(input, target, self.epsilon, group, valid, _on_device(self, input.device))
            if valid is None:
                return _FusedDiceFn.apply(input, target, self.epsilon, group)
            return _FusedDiceFn.apply(input, target, self.epsilon, group, valid)
        if self._torch.weight is not None and self._torch.weight.device != input.device:
            self._torch.to(input.device)
        return self._torch(input, target, valid)


class GeneralizedDiceLoss(nn.Module):
    """pytorch3dunet_losses.py:138-169: label contributions weighted by the inverse squared label volume."""

    def __init__(self, normalization="sigmoid", epsilon=1e-6):
        super().__init__()
        self.epsilon = epsilon
        self.normalization = {"sigmoid": torch.sigmoid, "softmax": lambda x: torch.softmax(x, 1), "none": lambda x: x}[normalization]

    def forward(self, input, target, valid=None):
        if valid is not None:
            input = _keep(input, _mask_like(valid, input))
        x, t = _per_channel(self.normalization(input)), _per_channel(target).float()
        if x.size(0) == 1:  # put foreground and background in separate channels
            x, t = torch.cat((x, 1 - x), 0), torch.cat((t, 1 - t), 0)
        if valid is not None:      # after the complement, so that 1 - p and 1 - t of an ignored pixel are left out too
            mask = (valid.reshape(1, -1) != 0)
            x, t = _keep(x, mask), _keep(t, mask)
        w = t.sum(-1)
        w = (1 / (w * w).clamp(min=self.epsilon)).detach()
        inter = ((x * t).sum(-1) * w).sum()
        denom = ((x + t).sum(-1) * w).clamp(min=self.epsilon).sum()
        return 1.0 - 2 * (inter / denom)


class BCEDiceLoss(nn.Module):
    """``weight``: K class weights for both terms (the reference gives its BCEDiceLoss none; its two parts take them)"""

    def __init__(self, alpha, beta, weight=None):
        super().__init__()
        self.alpha, self.beta = alpha, beta
        self.bce, self.dice = nn.BCEWithLogitsLoss(), DiceLoss(weight=class_weight_tensor(weight))

    @property
    def weight(self):
        return self.dice.weight

    def forward(self, input, target, valid=None):
        if valid is not None:
            return self.alpha * masked_bce_with_logits(input, target, valid, self.weight) + self.beta * self.dice(input, target, valid)
        if self.weight is not None:
            return self.alpha * weighted_bce_with_logits(input, target, self.weight) + self.beta * self.dice(input, target)
        return self.alpha * self.bce(input, target) + self.beta * self.dice(input, target)


class _FusedSegLossFn(torch.autograd.Function):
    """BCE-Dice / BCE / cross entropy / generalised Dice as one HIP reduction sweep + one gradient sweep (vs_seg_loss_fwd / _bwd)."""

    @staticmethod
    def forward(ctx, logits, targets, kind, alpha, beta, eps, valid=None, weight=None):
        from .. import _lib
        n, k = logits.shape[:2]
        hw = logits[0, 0].numel()
        logits = logits.contiguous()
        targets = targets.contiguous()
        is_f32 = targets.dtype == torch.float32
        if not is_f32 and targets.dtype != torch.uint8:
            targets, is_f32 = targets.float(), True
        if weight is not None:
            if weight.numel() != k:
                raise ValueError(f"{weight.numel()} class weights for {k} classes")
            nbytes = _lib.lib.vs_seg_loss_weighted_workspace(k)
        else:
            nbytes = _lib.lib.vs_seg_loss_workspace(k) if valid is None else _lib.lib.vs_seg_loss_masked_workspace(k)
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=logits.device)
        loss = torch.empty((), dtype=torch.float32, device=logits.device)
        if weight is not None:
            valid = None if valid is None else _valid_u8(valid, n, hw)
            _lib.check(_lib.lib.vs_seg_loss_fwd_weighted(kind, _lib.ptr(logits), _lib.ptr(targets), int(is_f32), _lib.ptr(valid),
                                                        _lib.ptr(weight), n, k, hw, float(alpha), float(beta), float(eps), _lib.ptr(loss),
                                                        _lib.ptr(ws), nbytes, _lib.stream_ptr()))
        elif valid is None:
            _lib.check(_lib.lib.vs_seg_loss_fwd(kind, _lib.ptr(logits), _lib.ptr(targets), int(is_f32), n, k, hw, float(alpha), float(beta),
                                               float(eps), _lib.ptr(loss), _lib.ptr(ws), nbytes, _lib.stream_ptr()))
        else:
            valid = _valid_u8(valid, n, hw)
            _lib.check(_lib.lib.vs_seg_loss_fwd_masked(kind, _lib.ptr(logits), _lib.ptr(targets), int(is_f32), _lib.ptr(valid), n, k, hw,
                                                      float(alpha), float(beta), float(eps), _lib.ptr(loss), _lib.ptr(ws), nbytes,
                                                      _lib.stream_ptr()))
        ctx.save_for_backward(logits, targets, ws, *(() if valid is None else (valid,)))
        ctx.class_weight = weight
        ctx.meta = (kind, n, k, hw, is_f32)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        from .. import _lib
        logits, targets, ws, *valid = ctx.saved_tensors
        kind, n, k, hw, is_f32 = ctx.meta
        dx = torch.empty_like(logits)
        g = grad_out.contiguous().float()
        if ctx.class_weight is not None:
            _lib.check(_lib.lib.vs_seg_loss_bwd_weighted(kind, _lib.ptr(logits), _lib.ptr(targets), int(is_f32),
                                                        _lib.ptr(valid[0] if valid else None), _lib.ptr(ctx.class_weight), _lib.ptr(g), n, k, hw,
                                                        _lib.ptr(ws), _lib.ptr(dx), _lib.stream_ptr()))
        elif not valid:
            _lib.check(_lib.lib.vs_seg_loss_bwd(kind, _lib.ptr(logits), _lib.ptr(targets), int(is_f32), _lib.ptr(g), n, k, hw, _lib.ptr(ws),
                                               _lib.ptr(dx), _lib.stream_ptr()))
        else:
            _lib.check(_lib.lib.vs_seg_loss_bwd_masked(kind, _lib.ptr(logits), _lib.ptr(targets), int(is_f32), _lib.ptr(valid[0]), _lib.ptr(g),
                                                      n, k, hw, _lib.ptr(ws), _lib.ptr(dx), _lib.stream_ptr()))
        return dx, None, None, None, None, None, None, None


class HipSegLoss(nn.Module):
    """The trainer's non-default criteria on GPU tensors (vol_seg_2d_trainer.py:124-148): ``kind`` in {"BCEDiceLoss", "BCELoss",
    "CrossEntropyLoss", "GeneralizedDiceLoss"}; one-hot targets (uint8 or float, the shape of the logits) - for the cross
    entropy the class index is the position of the 1 (the trainer's ``torch.argmax(targets, dim=1)``).  Anything the fused
    kernels do not take (CPU tensors, > 16 classes) goes through the torch restatement ``fallback``.  ``weight``: K class weights, used
    as given by both routes; the generalised Dice has its own inverse-volume weights and refuses them."""

    KINDS = {"BCEDiceLoss": 1, "BCELoss": 2, "CrossEntropyLoss": 3, "GeneralizedDiceLoss": 4}

    def __init__(self, kind: str, alpha: float = 1.0, beta: float = 1.0, epsilon: float = 1e-6, weight=None):
        super().__init__()
        self.kind, self.alpha, self.beta, self.epsilon = kind, alpha, beta, epsilon
        if weight is not None and kind == "GeneralizedDiceLoss":
            raise ValueError("GeneralizedDiceLoss has its own inverse-volume class weights and takes none")
        w = class_weight_tensor(weight)
        self.register_buffer("weight", w)
        if w is None:
            self.fallback = {"BCEDiceLoss": lambda: BCEDiceLoss(alpha, beta), "BCELoss": nn.BCEWithLogitsLoss,
                             "CrossEntropyLoss": nn.CrossEntropyLoss, "GeneralizedDiceLoss": lambda: GeneralizedDiceLoss(epsilon=epsilon)}[kind]()
        else:
            self.fallback = {"BCEDiceLoss": lambda: BCEDiceLoss(alpha, beta, weight=w),
                             "BCELoss": lambda: nn.BCEWithLogitsLoss(weight=w.clone().view(1, -1, 1, 1)),
                             "CrossEntropyLoss": lambda: nn.CrossEntropyLoss(weight=w.clone())}[kind]()

    def forward(self, input, target, valid=None):
        if (input.is_cuda and input.dtype == torch.float32 and input.dim() >= 3 and input.shape == target.shape
                and input.size(1) <= 16):
            if self.weight is not None:
                return _FusedSegLossFn.apply(input, target, self.KINDS[self.kind], self.alpha, self.beta, self.epsilon, valid,
                                             _on_device(self, input.device))
            if valid is None:
                return _FusedSegLossFn.apply(input, target, self.KINDS[self.kind], self.alpha, self.beta, self.epsilon)
            return _FusedSegLossFn.apply(input, target, self.KINDS[self.kind], self.alpha, self.beta, self.epsilon, valid)
        if self.weight is not None:
            self.fallback.to(input.device)
        if valid is not None:
            return masked_criterion(self.fallback, input, target, valid)
        if self.kind == "CrossEntropyLoss":
            return self.fallback(input, torch.argmax(target, dim=1))
        return self.fallback(input, target.float())


def masked_criterion(criterion, input, target, valid, weight=None):
    """One of the trainer's torch criteria on one-hot targets with a validity mask: the restatements of this module take the mask
    themselves, torch's own BCE-with-logits and cross entropy are replaced by their masked forms.  ``weight``: K class weights for
    those two; by default the ``weight`` the torch criterion was built with (the restatements carry their own)."""
    if isinstance(criterion, nn.BCEWithLogitsLoss):
        return masked_bce_with_logits(input, target, valid, criterion.weight if weight is None else weight)
    if isinstance(criterion, nn.CrossEntropyLoss):
        return masked_cross_entropy(input, target, valid, criterion.weight if weight is None else weight)
    return criterion(input, target.float(), valid)


class DiceCoefficient:
    def __init__(self, epsilon=1e-6, **kwargs):
        self.epsilon = epsilon

    def __call__(self, input, target, valid=None):
        return torch.mean(compute_per_channel_dice(input.flatten(2), target.flatten(2), epsilon=self.epsilon, valid=valid))


class MeanIoU:
    """Per-sample argmax one-hot, per-class Jaccard, mean over classes then samples (pytorch3dunet_metrics.py:34-106).
    Accepts the (N, C, 1, H, W) tensors the reference's trainer builds or plain (N, C, H, W).  GPU tensors go through
    one HIP sweep (vs_mean_iou); the torch ops below serve CPU tensors and the skip_channels / ignore_index options."""

    def from_logits(self, logits, target, valid=None):
        """metric(softmax(logits, dim=1), target) - the trainer's validation call - without materialising the softmax."""
        if (logits.is_cuda and logits.dtype == torch.float32 and logits.shape == target.shape and 1 < logits.size(1) <= 16
                and not self.skip_channels and self.ignore_index is None and target.dtype in (torch.uint8, torch.float32)):
            return self._hip(logits, target, from_logits=1, valid=valid)
        return self(torch.softmax(logits, dim=1), target, valid)

    @staticmethod
    def _hip(input, target, from_logits=0, valid=None):
        from .._lib import check, lib, ptr, stream_ptr
        n, c = input.size(0), input.size(1)
        x, t = input.contiguous(), target.contiguous()
        hw = x.numel() // (n * c)
        out = torch.empty((), dtype=torch.float32, device=x.device)
        if valid is not None:
            valid = _valid_u8(valid, n, hw)
            nbytes = lib.vs_mean_iou_masked_workspace(n, c)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
            check(lib.vs_mean_iou_masked(ptr(x), ptr(t), 1 if t.dtype == torch.float32 else 0, ptr(valid), from_logits, n, c, hw, ptr(out),
                                         ptr(ws), nbytes, stream_ptr()))
            return out
        nbytes = lib.vs_mean_iou_workspace(n, c)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        check(lib.vs_mean_iou(ptr(x), ptr(t), 1 if t.dtype == torch.float32 else 0, from_logits, n, c, hw, ptr(out), ptr(ws),
                              nbytes, stream_ptr()))
        return out

    def __init__(self, skip_channels=(), ignore_index=None, **kwargs):
        self.skip_channels, self.ignore_index = skip_channels, ignore_index

    def __call__(self, input, target, valid=None):
        """``valid``: intersection and union are counted over the valid pixels of each sample; a sample without one is left out of
        the mean over samples, and the result is NaN when no sample is left."""
        if (input.is_cuda and input.dtype == torch.float32 and input.shape == target.shape and input.size(1) <= 16
                and not self.skip_channels and self.ignore_index is None and target.dtype in (torch.uint8, torch.float32)):
            return self._hip(input, target, valid=valid)
        n_classes = input.size(1)
        scores = []
        for b, (p, t) in enumerate(zip(input, target)):
            if n_classes == 1:
                pred = (p > 0.5).to(torch.uint8)
            else:
                pred = torch.zeros_like(p, dtype=torch.uint8).scatter_(0, torch.argmax(p, dim=0, keepdim=True), 1)
            t = t.to(torch.uint8)
            if valid is not None:
                keep = (valid[b] != 0).reshape((1,) + tuple(t.shape[1:])).to(torch.uint8)
                if not bool(keep.any()):
                    continue
                pred, t = pred * keep, t * keep
            if self.ignore_index is not None:
                keep = t != self.ignore_index
                pred, t = pred * keep, t * keep
            ious = [torch.sum(pred[c] & t[c]).float() / torch.clamp(torch.sum(pred[c] | t[c]).float(), min=1e-8)
                    for c in range(n_classes) if c not in self.skip_channels]
            scores.append(torch.mean(torch.stack(ious)))
        if not scores:
            return torch.full((), float("nan"), device=input.device)
        return torch.mean(torch.stack(scores))
