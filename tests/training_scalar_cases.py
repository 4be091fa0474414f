"""What the tests of the training step's small kernels share (tests/test_training_scalars_host.py, tests/test_hip_training_scalars.py,
tools/training_scalar_probe.py): seeded inputs, float64 references, the bounds, and the figures (measured error, bound) that a test
asserts and the probe prints.  The kernels are csrc/loss.hip (default Dice, the four selectable criteria, MeanIoU, one-hot) and
csrc/optim.hip (AdamW, the per-step scalars of a recorded step).

References: the project's torch restatements (oracle.predictor_numpy.dice_loss_none, data/losses.py BCEDiceLoss and
GeneralizedDiceLoss, nn.BCEWithLogitsLoss, nn.CrossEntropyLoss on argmax(target, 1)) on float64 logits with float64 autograd -
anchored to the reference project's own numbers on g10_losses.npz by the host tests; oracle.predictor_numpy.mean_iou and
prepare_training_batch; and a NumPy float64 restatement of torch's single-tensor AdamW, anchored to torch.optim.AdamW.  (The
restatements convert the 0/1 targets to float32 before they meet the float64 logits: sums of ones are exact there up to 2^24 > every
n h w used here; the square of a label volume is rounded once, 6e-8, inside the generalised Dice weight.)

Every array is built once per process and never written to."""
import ctypes
import ctypes.util
import dataclasses
import functools

import numpy as np
import torch
from torch import nn

ALPHA, BETA, EPS = 0.75, 0.25, 1e-6          # BCEDiceLoss(alpha, beta) as g10 uses it; the epsilon of every Dice clamp
GRAD_OUT = 1.7                               # the factor the module route multiplies the loss by before .backward()
LOSS_BOUND, GRAD_BOUND = 2e-6, 2e-5          # |loss - ref| <= 2e-6 max(1, |ref|);  max|grad - ref| <= 2e-5 max|ref|  (no absolute term)
IOU_BOUND = 1e-6
MOMENT_BOUND, UPDATE_BOUND, UPDATE_ULPS = 5e-7, 8e-6, 1.5

CRITERIA = ("Dice", "BCEDiceLoss", "BCELoss", "CrossEntropyLoss", "GeneralizedDiceLoss")
SEG_KINDS = {"BCEDiceLoss": 1, "BCELoss": 2, "CrossEntropyLoss": 3, "GeneralizedDiceLoss": 4}

SHAPES = {"small_odd": (3, 33, 31), "one_wave": (1, 5, 7), "stride_odd": (1, 363, 363), "stride_vec": (5, 660, 640),
          "misaligned": (2, 32, 32)}


@dataclasses.dataclass(frozen=True)
class Case:
    """n x classes x h x w logits = scale * standard normal, labels uniform over max(classes, 2) values (one class: channel 0 of the
    two-value one-hot, as prepare_training_batch's output is sliced by the existing tests).
    absent: that class occurs in no sample (its pixels get the next label);  "last" = classes - 1.
    dead: what the network says about the absent class - "zero": logits exactly 0 (sum x^2 + sum t^2 = 0: the D <= eps branch of the
    default Dice), "off": logits -120 (sigmoid = 0 exactly in fp32: D <= eps of BCE-Dice; the clamped denominator term of the generalised
    Dice, `live` false), "faint": logits -40 (the same two branches without the exact zero, where one channel is all there is and
    every gradient must stay a normal fp32 number).
    saturate: rows 0..5 hold +-90 with random signs.  zero_column: every 7th pixel has no 1 in its one-hot column (a label value at or
    above `classes`)."""
    shape: str
    classes: int
    absent: object = None
    scale: float = 1.0
    tdtype: str = "uint8"
    dead: object = None
    saturate: bool = False
    zero_column: bool = False

    @property
    def nhw(self):
        return SHAPES[self.shape]

    @property
    def absent_class(self):
        return None if self.absent is None else (self.classes - 1 if self.absent == "last" else int(self.absent))

    @property
    def base(self):
        """the case the reference is computed for: the target dtype does not change the numbers"""
        return dataclasses.replace(self, tdtype="uint8")

    @property
    def id(self):
        parts = [self.shape, f"k{self.classes}", "u8" if self.tdtype == "uint8" else "f32"]
        if self.absent is not None:
            parts.append(f"absent-{self.absent}")
        if self.dead:
            parts.append(f"dead-{self.dead}")
        if self.scale != 1.0:
            parts.append(f"x{self.scale:g}")
        if self.saturate:
            parts.append("sat90")
        if self.zero_column:
            parts.append("zerocol")
        return "-".join(parts)


# The launch each case selects (csrc/loss.hip; reductions are 512 blocks x 256 threads = 131072 threads, 4 bytes each in the scalar
# kernels and 16 in the vector ones):
LOSS_CASES = (
    # hw = 1023, n k hw <= 49104: hw % 4 != 0 -> dice_partial_kernel / dice_grad_kernel (scalar), one trip, 8 workgroups with work and
    # a ragged last one; seg_partial / seg_grad one trip; class counts to the 16 that coef[16*4] and S[16][6] hold
    Case("small_odd", 1), Case("small_odd", 2), Case("small_odd", 3), Case("small_odd", 5), Case("small_odd", 16),
    # the same launches; a class that is in no sample: w = 1/eps in the generalised Dice, an all-zero target plane
    Case("small_odd", 1, absent=0),             # Dice 'none', one class, no foreground: the reference gradient is identically zero
    Case("small_odd", 3, absent=0), Case("small_odd", 3, absent="last"),
    Case("small_odd", 16, absent=0), Case("small_odd", 16, absent="last"),
    # .. and the network sure of it: D = 0 exactly (Dice gradients' D <= eps branch), `live` false in the generalised Dice
    Case("small_odd", 3, absent="last", dead="zero"), Case("small_odd", 3, absent="last", dead="off"),
    Case("small_odd", 1, absent=0, dead="zero"), Case("small_odd", 1, absent=0, dead="faint"),
    # the same launches; saturated sigmoid / softmax
    Case("small_odd", 1, scale=30.0), Case("small_odd", 3, scale=30.0), Case("small_odd", 3, saturate=True),
    # the <float> instantiations of the scalar kernels
    Case("small_odd", 1, tdtype="float32"), Case("small_odd", 3, tdtype="float32"),
    # cross entropy only: the all-zero one-hot column (`found` false in seg_partial_kernel and seg_grad_kernel)
    Case("small_odd", 3, zero_column=True), Case("small_odd", 3, zero_column=True, tdtype="float32"),
    # hw = 35 < 256: one workgroup has work and not all of it; n = 1
    Case("one_wave", 1), Case("one_wave", 3, tdtype="float32"),
    # hw = 131769 = 131072 + 697, odd: scalar kernels, threads 0..696 of the reductions take a second grid-stride trip
    Case("stride_odd", 2), Case("stride_odd", 3, tdtype="float32"),
    # hw = 422400 = 4 * 105600, n * 105600 = 528000 vectors: dice_partial4_kernel has all four loads of the first outer trip live
    # (4 * 131072 = 524288 < 528000, 105600 is no multiple of 131072: the loads cross sample boundaries) and threads 0..3711 take a second
    # outer trip with one live load.  dice_grad4_kernel: K = 2: 1056000 vectors, 2063 blocks, second vector live; K = 5: 2640000
    # vectors, the grid capped at 4096 blocks, second outer trip (2 * 1048576 < 2640000).  seg_grad_kernel: grid capped at 8192 blocks,
    # second trip for n k hw = 4224000 (K = 2) and, kind 3, for n hw = 2112000 > 2097152.  Both target types: <uint8_t> and <float>.
    Case("stride_vec", 2), Case("stride_vec", 2, tdtype="float32"), Case("stride_vec", 5), Case("stride_vec", 5, tdtype="float32"),
)


def criteria_of(case):
    """what runs on a case: the reference project offers no cross entropy on one channel (g10 has none either), and the zero-column
    cases are about the cross entropy alone"""
    if case.zero_column:
        return ("CrossEntropyLoss",)
    return tuple(c for c in CRITERIA if not (c == "CrossEntropyLoss" and case.classes == 1))


LOSS_PARAMS = [(case, crit) for case in LOSS_CASES for crit in criteria_of(case)]
# tests of one reference next to each other: the reference cache below holds a few entries
LOSS_PARAMS.sort(key=lambda cc: (LOSS_CASES.index(cc[0].base) if cc[0].base in LOSS_CASES else LOSS_CASES.index(cc[0]), CRITERIA.index(cc[1])))


def loss_id(param):
    return f"{param[0].id}-{param[1]}" if isinstance(param, tuple) else None


def _seed(case):
    n, h, w = case.nhw
    absent = -1 if case.absent_class is None else case.absent_class
    return [1000 + n, h, w, case.classes, absent + 1, int(case.scale), int(case.saturate), int(case.zero_column),
            {None: 0, "zero": 1, "off": 2, "faint": 3}[case.dead]]


@functools.lru_cache(maxsize=4)
def _base_inputs(case):
    """(logits float32 (n, k, h, w), one-hot uint8 (n, k, h, w)) of case.base"""
    n, h, w = case.nhw
    k, kk = case.classes, max(case.classes, 2)
    rng = np.random.default_rng(_seed(case))
    logits = (rng.standard_normal((n, k, h, w)) * case.scale).astype(np.float32)
    labels = rng.integers(0, kk, (n, h, w))
    c = case.absent_class
    if c is not None:
        labels[labels == c] = (c + 1) % kk
        if case.dead == "zero":
            logits[:, c] = 0.0
        elif case.dead in ("off", "faint"):
            logits[:, c] = -120.0 if case.dead == "off" else -40.0
    if case.saturate:
        logits[:, :, :6] = np.where(rng.integers(0, 2, (n, k, 6, w)) == 1, 90.0, -90.0).astype(np.float32)
    onehot = (labels[:, None] == np.arange(kk)[None, :, None, None])[:, :k].astype(np.uint8)
    if case.zero_column:
        flat = onehot.reshape(n, k, h * w)
        flat[:, :, ::7] = 0
    logits.setflags(write=False)
    onehot.setflags(write=False)
    return logits, onehot


def inputs(case):
    """(logits, targets) as numpy arrays, targets in the case's dtype"""
    logits, onehot = _base_inputs(case.base)
    return logits, (onehot if case.tdtype == "uint8" else onehot.astype(np.float32))


def criterion_fn(name):
    """the restatement of one criterion: f(logits, one-hot targets) -> scalar, any floating dtype of the logits"""
    from oracle import predictor_numpy as P
    from volume_segmantics_amd.data.losses import BCEDiceLoss, GeneralizedDiceLoss
    if name == "Dice":
        return lambda x, t: P.dice_loss_none(x, t, EPS)
    if name == "BCEDiceLoss":
        crit = BCEDiceLoss(ALPHA, BETA)
        return lambda x, t: crit(x, t.to(x.dtype))
    if name == "BCELoss":
        crit = nn.BCEWithLogitsLoss()
        return lambda x, t: crit(x, t.to(x.dtype))
    if name == "CrossEntropyLoss":
        crit = nn.CrossEntropyLoss()
        return lambda x, t: crit(x, torch.argmax(t, dim=1))
    if name == "GeneralizedDiceLoss":
        crit = GeneralizedDiceLoss(epsilon=EPS)
        return lambda x, t: crit(x, t)
    raise KeyError(name)


def evaluate(name, logits, targets, dtype):
    """(loss, d loss / d logits) of the restatement in `dtype`, as float and float64 array"""
    x = torch.tensor(np.asarray(logits)).to(dtype).requires_grad_()
    loss = criterion_fn(name)(x, torch.tensor(np.asarray(targets)))
    loss.backward()
    return float(loss.detach().double()), x.grad.double().numpy()


@functools.lru_cache(maxsize=4)
def _reference(case, name):
    logits, onehot = _base_inputs(case)
    loss, grad = evaluate(name, logits, onehot, torch.float64)
    grad.setflags(write=False)
    return loss, grad


def reference(case, name):
    """float64 (loss, gradient for grad_out = 1)"""
    return _reference(case.base, name)


def loss_errors(loss, grad, ref_loss, ref_grad, grad_out=1.0):
    """[(label, measured, bound)]: the two bounds every loss route is held to; grad was computed for the factor grad_out"""
    scale = float(np.abs(ref_grad).max())
    err = float(np.abs(np.asarray(grad, dtype=np.float64) - grad_out * ref_grad).max()) if np.isfinite(grad).all() else float("inf")
    return [("loss", abs(float(loss) - ref_loss), LOSS_BOUND * max(1.0, abs(ref_loss))),
            ("grad", err, GRAD_BOUND * grad_out * scale)]


# ---- the device side ---------------------------------------------------------------------------------------------------------------
DEV = "cuda:0"


def _offset_copy(array, offset):
    """device tensor holding `array`, its first element `offset` elements into a larger allocation (offset 0: the allocation itself)"""
    src = torch.tensor(np.ascontiguousarray(array)).reshape(-1)
    buf = torch.empty(src.numel() + 8, dtype=src.dtype, device=DEV)
    view = buf[offset:offset + src.numel()]
    view.copy_(src)
    return view


def abi_loss(name, logits, targets, grad_out=None, offsets=(0, 0, 0)):
    """vs_dice_loss_fwd/_bwd or vs_seg_loss_fwd/_bwd straight through the C ABI: (loss, dlogits) as numpy; dlogits is filled with NaN
    before the call, so an element no thread wrote stays NaN.  grad_out None: the null pointer.  offsets: elements by which the logits,
    targets and dlogits pointers are moved off their allocations."""
    from volume_segmantics_amd import _lib as L
    n, k = logits.shape[:2]
    hw = int(np.prod(logits.shape[2:]))
    is_f32 = int(targets.dtype == np.float32)
    x, t = _offset_copy(logits, offsets[0]), _offset_copy(targets, offsets[1])
    dbuf = torch.full((x.numel() + 8,), float("nan"), dtype=torch.float32, device=DEV)
    dx = dbuf[offsets[2]:offsets[2] + x.numel()]
    loss = torch.full((), float("nan"), dtype=torch.float32, device=DEV)
    g = None if grad_out is None else torch.tensor(float(grad_out), dtype=torch.float32, device=DEV)
    if name == "Dice":
        nbytes = L.lib.vs_dice_workspace(k)
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=DEV)
        L.check(L.lib.vs_dice_loss_fwd(L.ptr(x), L.ptr(t), is_f32, n, k, hw, EPS, L.ptr(loss), L.ptr(ws), nbytes, None))
        L.check(L.lib.vs_dice_loss_bwd(L.ptr(x), L.ptr(t), is_f32, L.ptr(g), n, k, hw, EPS, L.ptr(ws), L.ptr(dx), None))
    else:
        nbytes = L.lib.vs_seg_loss_workspace(k)
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=DEV)
        L.check(L.lib.vs_seg_loss_fwd(SEG_KINDS[name], L.ptr(x), L.ptr(t), is_f32, n, k, hw, ALPHA, BETA, EPS, L.ptr(loss), L.ptr(ws),
                                      nbytes, None))
        L.check(L.lib.vs_seg_loss_bwd(SEG_KINDS[name], L.ptr(x), L.ptr(t), is_f32, L.ptr(g), n, k, hw, L.ptr(ws), L.ptr(dx), None))
    torch.cuda.synchronize()
    guard = torch.cat([dbuf[:offsets[2]], dbuf[offsets[2] + x.numel():]])
    assert bool(torch.isnan(guard).all()), "dlogits written outside its n k h w elements"
    return loss.item(), dx.cpu().numpy().reshape(logits.shape)


def module_loss(name, logits, targets, grad_out=GRAD_OUT):
    """HipDiceLoss / HipSegLoss with autograd, the loss multiplied by grad_out before .backward(): (loss, logits.grad) as numpy"""
    from volume_segmantics_amd.data.losses import HipDiceLoss, HipSegLoss
    crit = HipDiceLoss(EPS) if name == "Dice" else HipSegLoss(name, ALPHA, BETA, EPS)
    x = torch.tensor(np.asarray(logits)).to(DEV).requires_grad_()
    loss = crit(x, torch.tensor(np.asarray(targets)).to(DEV))
    assert loss.is_cuda
    (loss * grad_out).backward()
    torch.cuda.synchronize()
    return loss.item(), x.grad.cpu().numpy()


def loss_figures(case, name):
    """both routes of one (case, criterion): the module with grad_out = 1.7, the C ABI with the null grad_out"""
    logits, targets = inputs(case)
    ref_loss, ref_grad = reference(case, name)
    out = []
    loss, grad = module_loss(name, logits, targets)
    out += [(f"module {label}", err, bound) for label, err, bound in loss_errors(loss, grad, ref_loss, ref_grad, GRAD_OUT)]
    loss, grad = abi_loss(name, logits, targets)
    out += [(f"abi {label}", err, bound) for label, err, bound in loss_errors(loss, grad, ref_loss, ref_grad)]
    return out


# pointer offsets (logits, targets, dlogits) in elements, on hw = 1024: each must make vs_dice_loss_fwd / _bwd refuse the 16-byte kernels
MISALIGNED = {"logits+1float": ("uint8", (1, 0, 0)), "u8target+1byte": ("uint8", (0, 1, 0)), "f32target+1float": ("float32", (0, 1, 0)),
              "dlogits+1float": ("uint8", (0, 0, 1)), "u8target+2bytes-logits+2floats": ("uint8", (2, 2, 2))}


# ---- MeanIoU ---------------------------------------------------------------------------------------------------------------------
IOU_CLASSES = (1, 2, 3, 7, 16)
IOU_SHAPES = ("small_odd", "stride_odd")     # hw = 1023: 4 blocks per sample; hw = 131769: grid capped at 64 blocks, stride 16384, 9 trips


@functools.lru_cache(maxsize=None)
def iou_inputs(shape, classes):
    """(logits, probabilities, one-hot uint8, reference).  Logits are standard normal rounded to multiples of 1/8: two logits are equal
    (an exact tie, in expf as in torch's exp: the first maximum wins) or at least 1/8 apart (probabilities a factor 1.13 apart) - no
    pair whose fp32 probabilities could round equal in one implementation and not in the other.  Rows 0..3 of sample 0 are all-equal."""
    from oracle import predictor_numpy as P
    n, h, w = SHAPES[shape]
    rng = np.random.default_rng([2000 + n, h, w, classes])
    logits = (np.round(rng.standard_normal((n, classes, h, w)) * 8.0) / 8.0).astype(np.float32)
    logits[0, :, :4] = 0.25
    logits[0, :, 4:6] = -3.0                                          # one channel: sigmoid < 0.5, nothing predicted
    x = torch.from_numpy(logits)
    probs = torch.softmax(x, 1) if classes > 1 else torch.sigmoid(x)
    labels = rng.integers(0, max(classes, 2), (n, h, w))
    onehot = torch.from_numpy((labels[:, None] == np.arange(max(classes, 2))[None, :, None, None])[:, :classes].astype(np.uint8))
    return x, probs, onehot, float(P.mean_iou(probs, onehot))


def iou_figures(shape, classes, tdtype):
    from volume_segmantics_amd.data.losses import MeanIoU
    x, probs, onehot, ref = iou_inputs(shape, classes)
    t = (onehot if tdtype == "uint8" else onehot.float()).to(DEV)
    got = MeanIoU()(probs.to(DEV), t)
    got_logits = MeanIoU().from_logits(x.to(DEV), t)           # one channel: softmax = 1 everywhere, through the same kernel
    ref_logits = ref if classes > 1 else float(_iou_one_channel_softmax(onehot))
    assert got.is_cuda and got_logits.is_cuda
    return [("probabilities", abs(got.item() - ref), IOU_BOUND), ("from_logits", abs(got_logits.item() - ref_logits), IOU_BOUND)]


def _iou_one_channel_softmax(onehot):
    from oracle import predictor_numpy as P
    return P.mean_iou(torch.ones(onehot.shape), onehot)


# ---- one-hot ---------------------------------------------------------------------------------------------------------------------
# hw = 1023: the scalar branch of onehot_kernel for every group of four; hw = 35: one block, ragged; hw = 422400 = 4 * 105600: the
# uchar4 branch, grid 256 blocks x 256 threads = 65536 vectors per trip -> a second trip
ONEHOT_SHAPES = ("small_odd", "one_wave", "stride_vec")
ONEHOT_CLASSES = (2, 7, 255)


def onehot_labels(shape, classes):
    """uint8 labels (n, h, w) over 0..classes+2 capped at 255: values at or above `classes` occur wherever they fit in a byte (the
    first two pixels hold `classes` and `classes - 1`, so both sides of the edge are there at any size)"""
    n, h, w = SHAPES[shape]
    rng = np.random.default_rng([3000 + n, h, w, classes])
    labels = rng.integers(0, min(classes + 3, 256), (n, h, w)).astype(np.uint8)
    labels[0, 0, :2] = (classes, classes - 1)
    return labels


def onehot_reference(labels, classes, rows=64):
    """prepare_training_batch on 256 label values, cut to the first `classes` channels: a label at or above `classes` leaves its column
    zero.  In slabs of rows, so the int64 one-hot torch builds on the way stays small."""
    from oracle import predictor_numpy as P
    lab = torch.tensor(labels)
    out = torch.empty((lab.shape[0], classes) + tuple(lab.shape[1:]), dtype=torch.uint8)
    for r in range(0, lab.shape[1], rows):
        out[:, :, r:r + rows] = P.prepare_training_batch(None, lab[:, r:r + rows], 256)[1][:, :classes]
    return out


def onehot_device(labels, classes):
    from volume_segmantics_amd import _lib as L
    lab = torch.tensor(labels).to(DEV)
    n, hw = lab.shape[0], lab[0].numel()
    out = torch.full((n, classes) + tuple(lab.shape[1:]), 0xAB, dtype=torch.uint8, device=DEV)
    L.check(L.lib.vs_onehot_u8(L.ptr(lab), n, classes, hw, L.ptr(out), None))
    torch.cuda.synchronize()
    return out


# ---- AdamW -----------------------------------------------------------------------------------------------------------------------
def f32(value):
    """the value that crosses the C ABI in a float argument"""
    return float(np.float32(value))


def adamw_reference(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, mask=None):
    """torch.optim.AdamW, single-tensor path, in float64: (p, m, v) after the step.  The scalars are used as given: hand it
    f32(0.999), not 0.999, to share the kernel's betas.  mask (optional): elements with mask == 0 are left alone."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    p1 = p * (1.0 - lr * weight_decay)
    m1 = beta1 * m + (1.0 - beta1) * g
    v1 = beta2 * v + (1.0 - beta2) * g * g
    bias1 = 1.0 - beta1 ** step
    bias2_sqrt = np.sqrt(1.0 - beta2 ** step)
    p1 = p1 - (lr / bias1) * (m1 / (np.sqrt(v1) / bias2_sqrt + eps))
    if mask is not None:
        keep = np.asarray(mask) != 0
        p1, m1, v1 = np.where(keep, p1, p), np.where(keep, m1, m), np.where(keep, v1, v)
    return p1, m1, v1


ADAMW_SIZES = (1, 8192 * 256 + 10007)         # adamw_kernel: grid capped at 8192 blocks x 256 threads; 10007 elements take a second trip
ADAMW_BETA2, ADAMW_EPS, ADAMW_WD = 0.999, 1e-8, 0.01
# (step, lr, beta1, masked): six consecutive steps of a OneCycle-like schedule (lr up, beta1 down, then back), then two late ones
ADAMW_SCHEDULE = ((1, 4e-5, 0.95, False), (2, 3e-4, 0.92, False), (3, 1e-3, 0.85, True), (4, 7e-4, 0.88, False), (5, 2e-4, 0.93, True),
                  (6, 1e-5, 0.95, True), (1000, 5e-4, 0.9, False), (100000, 1e-6, 0.95, True))


@functools.lru_cache(maxsize=None)
def adamw_inputs(n):
    """p0 float32, mask uint8, and one gradient per schedule entry.  Every element keeps the sign of its gradient through the run, so
    exp_avg = beta1 m + (1 - beta1) g never cancels and 'relative to the reference' is a bound a correctly rounded kernel can meet; an
    element's magnitude is drawn anew each step, log-uniform over 1e-12 .. 1e3, and one in sixteen gradients is exactly zero."""
    rng = np.random.default_rng([4000, n])
    p0 = rng.standard_normal(n).astype(np.float32)
    sign = np.where(rng.integers(0, 2, n) == 1, 1.0, -1.0)
    mask = (rng.random(n) > 0.3).astype(np.uint8)
    grads = []
    for _ in ADAMW_SCHEDULE:
        g = (sign * 10.0 ** rng.uniform(-12.0, 3.0, n)).astype(np.float32)
        g[rng.integers(0, 16, n) == 0] = 0.0
        grads.append(g)
    if n > 4:
        grads[0][:4] = (1e-12, -1e-12, 1e3, -1e3)
        for g in grads[1:]:
            g[:4] = np.abs(g[:4]) * (1, -1, 1, -1)
    return p0, mask, grads


def adamw_step_figures(before, after, g, hyper, step, mask):
    """[(label, measured / bound)] worst over the elements, for one step from the device state `before` = (p, m, v) to `after`; and the
    count of masked elements whose bits changed.  exp_avg, exp_avg_sq: |got - ref| <= 5e-7 |ref|.  Update: Delta p = p_after - p_before
    in float64 from the device values against the reference's, <= 8e-6 |Delta p_ref| + 1.5 ulp(p), ulp(p) the fp32 spacing at the larger
    of |p_before| and |p_after|."""
    lr, b1, b2, eps, wd = hyper
    ref = adamw_reference(before[0], g, before[1], before[2], lr, b1, b2, eps, wd, step, mask)
    out = []
    for label, got, want in (("exp_avg", after[1], ref[1]), ("exp_avg_sq", after[2], ref[2])):
        err, bound = np.abs(got.astype(np.float64) - want), MOMENT_BOUND * np.abs(want)
        out.append((label, _worst_ratio(err, bound)))
    delta = after[0].astype(np.float64) - before[0].astype(np.float64)
    delta_ref = ref[0] - before[0].astype(np.float64)
    ulp = np.spacing(np.maximum(np.abs(before[0]), np.abs(after[0])).astype(np.float32)).astype(np.float64)
    out.append(("update", _worst_ratio(np.abs(delta - delta_ref), UPDATE_BOUND * np.abs(delta_ref) + UPDATE_ULPS * ulp)))
    changed = 0
    if mask is not None:
        frozen = np.asarray(mask) == 0
        changed = sum(int((a[frozen].view(np.uint32) != b[frozen].view(np.uint32)).sum()) for a, b in zip(after, before))
    return out, changed


def _worst_ratio(err, bound):
    """max err / bound; an error above a zero bound is infinite, a zero error on a zero bound is 0"""
    if not np.isfinite(err).all():
        return float("inf")
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0.0, 0.0, err / bound)
    return float(ratio.max())


def adamw_run(n):
    """the schedule on the device, one vs_adamw_step per entry: yields (step, [(label, ratio)], changed masked elements)"""
    from volume_segmantics_amd import _lib as L
    p0, mask, grads = adamw_inputs(n)
    p, m, v = torch.tensor(p0).to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    mask_d = torch.from_numpy(mask).to(DEV)
    b2, eps, wd = f32(ADAMW_BETA2), f32(ADAMW_EPS), f32(ADAMW_WD)
    for (step, lr, b1, masked), g in zip(ADAMW_SCHEDULE, grads):
        lr, b1 = f32(lr), f32(b1)
        before = [a.cpu().numpy() for a in (p, m, v)]
        gd = torch.from_numpy(g).to(DEV)
        L.check(L.lib.vs_adamw_step(L.ptr(p), L.ptr(gd), L.ptr(m), L.ptr(v), L.ptr(mask_d) if masked else None, n, lr, b1, b2, eps, wd,
                                    step, None))
        torch.cuda.synchronize()
        after = [a.cpu().numpy() for a in (p, m, v)]
        figures, changed = adamw_step_figures(before, after, g, (lr, b1, b2, eps, wd), step, mask if masked else None)
        yield step, figures, changed


# ---- vs_train_hyper_set ----------------------------------------------------------------------------------------------------------
def host_hyper(lr, beta1, beta2, eps, weight_decay, step):
    """the eight floats as the host computes them in float32: powf of the C library (the function the shared library calls), a
    correctly rounded subtraction and square root"""
    libm = ctypes.CDLL(ctypes.util.find_library("m"))
    libm.powf.restype, libm.powf.argtypes = ctypes.c_float, [ctypes.c_float, ctypes.c_float]
    one = np.float32(1.0)
    bias1 = one - np.float32(libm.powf(beta1, float(step)))
    bias2_sqrt = np.sqrt(one - np.float32(libm.powf(beta2, float(step))))
    return np.array([lr, beta1, beta2, eps, weight_decay, bias1, bias2_sqrt, step], dtype=np.float32)


HYPER_CASES = ((1e-3, 0.9, 0.999, 1e-8, 0.01, 1), (3e-4, 0.85, 0.99, 1e-8, 0.0, 7), (5e-4, 0.95, 0.999, 1e-6, 0.05, 1000),
               (1e-6, 0.9, 0.999, 1e-8, 0.01, 100000))
