"""What the convolution tests share (tests/test_conv_host.py, tests/test_hip_conv_bounds.py, and the helpers of tests/test_hip_ops.py and
tests/test_hip_ring_kernels.py): the table of cases - one row per kernel instantiation the forward launch of csrc/conv_igemm.hip can
select, with the plan code written out by hand - seeded inputs, the float64 reference, the per-element bound with its derivation, and
the figure (measured error over bound) a test asserts to be at most 1.

Covered: launch_conv_igemm's forward launch - every tile instantiation of launch_tile without normalise-on-load, the ring kernel's
three modes, the persistent stream kernel at both cout tiles, the direct strip kernel and the head kernel - with the loader forms
(nearest x2 + concatenation, zero stuffing, dilation) and the epilogue forms (affine, shift, residual, ReLU, fp32 / NCHW store, 2 x 2
sum-pool, split output).  The weight gradients have their own table of this kind, tests/wgrad_cases.py, and so has the stem
(csrc/stem.hip, forward and weight gradient), tests/stem_cases.py.  Not covered here: the BatchNorm-backward epilogue (bz),
normalise-on-load, swish, grouped and depthwise forms; they keep their own tests.

The bound, per output element.  U = 2^-24 is the unit roundoff of fp32, gamma_m = m U / (1 - m U) bounds m roundings in a row.  The
inputs are fp32 values the storage type holds exactly, so no input rounding is charged.  Every later term is taken on the magnitude
that flows through it: |value of the float64 reference at that point| + the error accumulated so far.

  accumulation  S = conv(|x|, |w|) over the source as the loader defines it, K = taps * (c0 + c1) products per output.
                fp32: the accumulator is one chain acc = fma(a, b, acc) over the K products in k order (v_mfma_f32_16x16x4_f32: exact
                product, one rounding per step) - K roundings, gamma_K S.
                bf16 / fp16: the products of 16-bit operands are exact in fp32, but how v_mfma_f32_16x16x32 sums its 32 products is
                not documented, so each product is charged two roundings (one inside the instruction, one when the instruction's sum
                joins the accumulator) - gamma_2K S.  Any summation order of K terms in which a term meets at most 2K roundings
                stays below it.
  pooled form   four accumulators are summed (conv_epilogue: acc + acc, then + the neighbour lane; conv_direct_kernel MODE 1 the
                same): the four accumulation bounds add, and three fp32 adds are charged on sum |A_i| + their error - gamma_3.
  scale         v * scale: the error so far is multiplied by |scale|, one rounding.
  shift         + shift: one rounding (a fused v * scale + shift rounds once; two are charged).
  residual      + residual (a value the storage type holds exactly): one rounding.
  ReLU          max(v, 0) is exact and 1-Lipschitz: the bound carries over unchanged, no element is left out.
  store         half a unit in the last place of the stored type: 2^-8 relative for bf16, 2^-11 for fp16, U for fp32 and out_f32
                (an fp32 store rounds nothing: U is charged all the same), never less than half the type's smallest subnormal step
                (2^-134, 2^-25, 2^-150) - the one absolute term, a property of the format.
There is no other absolute slack and no measured constant."""
import dataclasses
import functools
import math

import torch
import torch.nn.functional as F

from hip_helpers import conv_desc, option, rounded, tol

U = 2.0 ** -24
STORE = {0: (2.0 ** -24, 2.0 ** -150), 1: (2.0 ** -8, 2.0 ** -134), 2: (2.0 ** -11, 2.0 ** -25)}    # (relative half ulp, half the subnormal step)
CHUNK = {0: 16, 1: 32, 2: 32}          # input channels per staged chunk (conv_common.h: CT<T>::CK)
DT = {0: "fp32", 1: "bf16", 2: "fp16"}


def gamma(m):
    """m roundings in a row: (1 + U)^m - 1 <= m U / (1 - m U)"""
    return m * U / (1.0 - m * U)


# ---- the table ------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Case:
    """h, w: the virtual input (after the loader's x2); pad = dilation * (k // 2).  inst: which instantiation the row stands for -
    the tuple (BN, PT, NW, taps, stride, dilation) of launch_tile, or ("ring", mode) / ("stream", BN) / ("direct",) / ("direct-up0",) /
    ("head",); None for the rows that run a loader or epilogue form on an instantiation another row already stands for."""
    label: str
    code: int                    # 0 = fp32, 1 = bf16, 2 = fp16
    n: int
    h: int
    w: int
    c0: int
    cout: int
    k: int = 3
    stride: int = 1
    dilation: int = 1
    c1: int = 0
    up0: int = 0
    affine: int = 0
    bias: int = 0                # shift only
    residual: int = 0
    relu: int = 0
    out_f32: int = 0             # 0, or 3 = fp32 NCHW (the head)
    pool0: int = 0
    split_c: int = 0
    options: tuple = ()          # ((name, value), ...) for hip_helpers.option
    plan: int = 0                # what vs_conv2d_variant / vs_conv2d_train_variant must answer
    inst: tuple = None
    stat_rows: int = 0           # ring rows: what vs_conv2d_stat_rows must answer (tells mode 2 from mode 3)

    @property
    def id(self):
        return f"{self.label}-{DT[self.code]}"

    @property
    def pad(self):
        return self.dilation * (self.k // 2)

    @property
    def hout(self):
        return (self.h + 2 * self.pad - (self.k - 1) * self.dilation - 1) // self.stride + 1

    @property
    def wout(self):
        return (self.w + 2 * self.pad - (self.k - 1) * self.dilation - 1) // self.stride + 1

    @property
    def cin(self):
        return self.c0 + self.c1

    @property
    def seed(self):
        return sum(ord(ch) * (i + 1) for i, ch in enumerate(self.id)) % 100003

    @property
    def store_code(self):
        return 0 if self.out_f32 else self.code

    @property
    def family(self):
        return {1: "tile", 2: "tile", 8: "tile", 4: "direct", 6: "ring", 7: "stream"}[self.plan % 10]


ALL3, HALF, TRAIN = (0, 1, 2), (1, 2), (0, 1)
SMALL = (("conv_min_wgs", 1), ("conv_nw8_min_wgs", 1))      # no workgroup floors: small launches keep the wide tiles
NW4 = SMALL + (("conv_nw8", 0),)
STREAM = (("conv_stream_min_tiles", 1),)
DIRECT = (("conv_direct_min_px", 1), ("conv_direct_rows", 6))

# The tile family: (instantiation, (n, h, w), cout, k, stride, dilation, options, plan code).  c0 = 40: 32 + 8 for the 16-bit types,
# 16 + 16 + 8 for fp32.  Tiles: 16 x 16 pixels at 8 waves, 8 x 16 at 4 waves x 2, 8 x 8 at 4 waves x 1; cout tiles 64 / 32 / 16.
TILE_ROWS = [
    ((64, 2, 8, 9, 1, 1), (3, 20, 36), 72, 3, 1, 1, SMALL, 64298),
    ((32, 2, 8, 9, 1, 1), (3, 20, 36), 40, 3, 1, 1, SMALL, 32298),
    ((16, 2, 8, 9, 1, 1), (3, 20, 36), 20, 3, 1, 1, SMALL, 16298),
    ((64, 2, 8, 1, 1, 1), (3, 20, 36), 72, 1, 1, 1, SMALL, 64218),
    ((32, 2, 8, 1, 1, 1), (3, 20, 36), 40, 1, 1, 1, SMALL, 32218),
    ((16, 2, 8, 1, 1, 1), (3, 20, 36), 20, 1, 1, 1, SMALL, 16218),
    ((64, 1, 4, 9, 1, 1), (3, 20, 12), 72, 3, 1, 1, SMALL, 64191),
    ((32, 1, 4, 9, 1, 1), (3, 20, 12), 40, 3, 1, 1, SMALL, 32191),
    ((16, 1, 4, 9, 1, 1), (3, 20, 12), 20, 3, 1, 1, SMALL, 16191),
    ((64, 1, 4, 1, 1, 1), (3, 7, 9), 72, 1, 1, 1, SMALL, 64111),
    ((32, 1, 4, 1, 1, 1), (3, 7, 9), 40, 1, 1, 1, SMALL, 32111),
    ((16, 1, 4, 1, 1, 1), (3, 7, 9), 20, 1, 1, 1, SMALL, 16111),
    ((64, 2, 4, 9, 1, 1), (3, 20, 36), 72, 3, 1, 1, NW4, 64291),
    ((32, 2, 4, 9, 1, 1), (3, 20, 36), 40, 3, 1, 1, NW4, 32291),
    ((16, 2, 4, 9, 1, 1), (3, 20, 36), 20, 3, 1, 1, NW4, 16291),
    ((64, 2, 4, 1, 1, 1), (3, 20, 36), 72, 1, 1, 1, NW4, 64211),
    ((32, 2, 4, 1, 1, 1), (3, 20, 36), 40, 1, 1, 1, NW4, 32211),
    ((16, 2, 4, 1, 1, 1), (3, 20, 36), 20, 1, 1, 1, NW4, 16211),
    ((64, 1, 4, 9, 2, 1), (3, 19, 23), 72, 3, 2, 1, SMALL, 64192),
    ((32, 1, 4, 9, 2, 1), (3, 19, 23), 40, 3, 2, 1, SMALL, 32192),
    ((16, 1, 4, 9, 2, 1), (3, 19, 23), 20, 3, 2, 1, SMALL, 16192),
    ((64, 1, 4, 1, 2, 1), (3, 19, 23), 72, 1, 2, 1, SMALL, 64112),
    ((32, 1, 4, 1, 2, 1), (3, 19, 23), 40, 1, 2, 1, SMALL, 32112),
    ((16, 1, 4, 1, 2, 1), (3, 19, 23), 20, 1, 2, 1, SMALL, 16112),
    ((64, 2, 4, 9, 2, 1), (2, 24, 40), 72, 3, 2, 1, SMALL, 64292),
    ((64, 2, 4, 9, 1, 2), (2, 20, 36), 72, 3, 1, 2, SMALL, 64291),
    ((32, 2, 4, 9, 1, 2), (2, 20, 36), 40, 3, 1, 2, SMALL, 32291),
    ((64, 1, 4, 9, 1, 2), (2, 20, 12), 72, 3, 1, 2, SMALL, 64191),
    ((32, 1, 4, 9, 1, 2), (2, 20, 12), 40, 3, 1, 2, SMALL, 32191),
    ((64, 2, 4, 9, 1, 4), (2, 20, 36), 72, 3, 1, 4, SMALL, 64291),
    ((32, 2, 4, 9, 1, 4), (2, 20, 36), 40, 3, 1, 4, SMALL, 32291),
    ((64, 1, 4, 9, 1, 4), (2, 20, 12), 72, 3, 1, 4, SMALL, 64191),
    ((32, 1, 4, 9, 1, 4), (2, 20, 12), 40, 3, 1, 4, SMALL, 32191),
]


def _tile_cases():
    out = []
    for inst, (n, h, w), cout, k, stride, dil, opts, plan in TILE_ROWS:
        bn, pt, nw, taps, st, d = inst
        label = f"tile{bn}x{pt}x{nw}-k{k}s{stride}d{dil}-{n}x{h}x{w}x40to{cout}"
        out += [Case(label, code, n, h, w, 40, cout, k=k, stride=stride, dilation=dil, options=opts, plan=plan, inst=inst) for code in ALL3]
    return out


def _over(codes, label, *a, **kw):
    return [Case(label, code, *a, **kw) for code in codes]


# the loader and epilogue forms on the 8-wave tile kernel (3 x 20 x 36, 64298)
_T = dict(options=SMALL, plan=64298)
TILE_FORMS = (
    _over(ALL3, "tile-up1+concat-3x20x36x32+40to72", 3, 20, 36, 32, 72, c1=40, up0=1, **_T) +
    _over(ALL3, "tile-stuffed-3x20x36x40to72", 3, 20, 36, 40, 72, up0=2, **_T) +
    _over(ALL3, "tile-stuffed-1x1-3x20x36x40to72", 3, 20, 36, 40, 72, k=1, up0=2, options=SMALL, plan=64218) +
    _over(ALL3, "tile-affine+residual+relu-3x20x36x40to72", 3, 20, 36, 40, 72, affine=1, residual=1, relu=1, **_T) +
    _over(ALL3, "tile-shift-3x20x36x40to72", 3, 20, 36, 40, 72, bias=1, **_T) +
    _over(ALL3, "tile-relu-3x20x36x40to72", 3, 20, 36, 40, 72, relu=1, **_T) +
    _over(TRAIN, "tile-pooled-3x20x36x40to72", 3, 20, 36, 40, 72, pool0=1, **_T) +
    _over(ALL3, "tile-split64-3x20x36x40to72", 3, 20, 36, 40, 72, split_c=64, **_T))

# the ring kernel (bf16, default options): its workgroup floors are 224 (mode 1, 64 couts) and 128 (mode 2, 32 couts)
RING = [
    Case("ring1-7x56x72x136to72", 1, 7, 56, 72, 136, 72, plan=64296, inst=("ring", 1), stat_rows=140),
    Case("ring2-6x40x72x136to40", 1, 6, 40, 72, 136, 40, plan=32296, inst=("ring", 2), stat_rows=90),
    Case("ring3-2x8x8x136to40", 1, 2, 8, 8, 136, 40, plan=32296, inst=("ring", 3), stat_rows=1),
]
_R = dict(plan=32296, stat_rows=90)
RING_FORMS = [
    Case("ring2-up1+concat-6x40x72x96+40to40", 1, 6, 40, 72, 96, 40, c1=40, up0=1, **_R),
    Case("ring2-stuffed-6x40x72x136to40", 1, 6, 40, 72, 136, 40, up0=2, **_R),
    Case("ring2-affine+residual+relu-6x40x72x136to40", 1, 6, 40, 72, 136, 40, affine=1, residual=1, relu=1, **_R),
    Case("ring2-shift-6x40x72x136to40", 1, 6, 40, 72, 136, 40, bias=1, **_R),
    Case("ring2-pooled-6x40x72x136to40", 1, 6, 40, 72, 136, 40, pool0=1, **_R),
    Case("ring2-split32-6x40x72x136to40", 1, 6, 40, 72, 136, 40, split_c=32, **_R),
    Case("ring3-affine+residual+relu-2x8x8x136to40", 1, 2, 8, 8, 136, 40, affine=1, residual=1, relu=1, plan=32296, stat_rows=1),
]

# the persistent stream kernel: 256 tile jobs of 16 x 16 pixels x one cout tile at the least (conv_stream_min_tiles = 1), input
# channels in whole chunks of 32, couts a multiple of 32.  40 x 56 = 2.5 x 3.5 tiles is the ragged shape.
STREAM_CASES = (
    _over(HALF, "stream64-16x64x64x64to64", 16, 64, 64, 64, 64, options=STREAM, plan=64297, inst=("stream", 64)) +
    _over(HALF, "stream32-ragged-8x40x56x64to96", 8, 40, 56, 64, 96, options=STREAM, plan=32297, inst=("stream", 32)) +
    _over(HALF, "stream64-ragged-up1+concat-11x40x56x32+32to128", 11, 40, 56, 32, 128, c1=32, up0=1, options=STREAM, plan=64297) +
    _over(HALF, "stream32-ragged-affine+residual+relu-8x40x56x64to96", 8, 40, 56, 64, 96, affine=1, residual=1, relu=1, options=STREAM, plan=32297))

# the direct strip kernel (strips of 16 columns x 6 rows) and the head kernel; fp32 where direct_ok admits it (c0 <= 16)
_D = dict(options=DIRECT, plan=16294)
DIRECT_CASES = (
    _over(HALF, "direct-2x21x37x24to12", 2, 21, 37, 24, 12, inst=("direct",), **_D) +
    [Case("direct-2x21x37x12to12", 0, 2, 21, 37, 12, 12, inst=("direct",), **_D)] +
    _over(ALL3, "direct-up1-2x22x38x8to16", 2, 22, 38, 8, 16, up0=1, inst=("direct-up0",), **_D) +
    _over(ALL3, "head-2x21x37x16to3", 2, 21, 37, 16, 3, bias=1, out_f32=3, inst=("head",), **_D) +
    _over(ALL3, "direct-affine+relu-2x21x37x16to12", 2, 21, 37, 16, 12, affine=1, relu=1, **_D) +
    _over(ALL3, "direct-shift-2x21x37x16to12", 2, 21, 37, 16, 12, bias=1, **_D) +
    _over(TRAIN, "direct-pooled-2x22x38x16to8", 2, 22, 38, 16, 8, pool0=1, **_D))

CASES = _tile_cases() + TILE_FORMS + RING + RING_FORMS + STREAM_CASES + DIRECT_CASES

# vs_conv2d_variant answers 16191 for a dilated 16-channel layer; dispatch has no such kernel and must refuse it
REJECTED = [Case("dilated-16-rejected-2x20x12x40to20", code, 2, 20, 12, 40, 20, dilation=2, options=SMALL, plan=16191) for code in ALL3]


# ---- the launch of a case (host logic: the queries run without a GPU) ----------------------------------------------------------------
def descriptor(L, case):
    return conv_desc(L, case.code, case.n, case.h, case.w, case.c0, case.cout, case.k, case.stride, case.pad, c1=case.c1, up0=case.up0,
                     relu=case.relu, out_f32=case.out_f32, split_c=case.split_c, dilation=case.dilation if case.dilation > 1 else 0)


def train_block(L, case):
    t = L.ConvTrain()
    t.pool0 = case.pool0
    return t


def queried(L, case):
    """(plan code, partial rows) the library answers for the case under the case's options; the pooled form asks the training query"""
    with option(**dict(case.options)):
        d, t = descriptor(L, case), train_block(L, case)
        code = L.lib.vs_conv2d_train_variant(d, t) if case.pool0 else L.lib.vs_conv2d_variant(d)
        return code, L.lib.vs_conv2d_stat_rows(d, t)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def inputs(case):
    """x0 (the stored source: half resolution when up0), x1 or None, w (cout, cin, k, k), scale, shift, residual or None - fp32 CPU
    tensors in NCHW whose values the case's dtype holds exactly (scale and shift are fp32 as the launch takes them)."""
    g = torch.Generator().manual_seed(case.seed)
    sh = 1 if case.up0 else 0
    x0 = rounded(torch.randn(case.n, case.c0, case.h >> sh, case.w >> sh, generator=g), case.code)
    x1 = rounded(torch.randn(case.n, case.c1, case.h, case.w, generator=g), case.code) if case.c1 else None
    kk = case.k * case.k * case.cin
    w = rounded(torch.randn(case.cout, case.cin, case.k, case.k, generator=g) / kk ** 0.5, case.code)
    scale = torch.rand(case.cout, generator=g) + 0.5 if case.affine else None
    shift = torch.randn(case.cout, generator=g) if (case.affine or case.bias) else None
    res = rounded(torch.randn(case.n, case.cout, case.hout, case.wout, generator=g), case.code) if case.residual else None
    return x0, x1, w, scale, shift, res


# ---- the reference and the bound ---------------------------------------------------------------------------------------------------
def source(x0, x1, up0):
    """the tensor the loader defines: nearest x2 (up0 = 1) or zero stuffing (up0 = 2) of x0, then the concat partner; in x0's dtype"""
    v = x0
    if up0 == 1:
        v = v.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    elif up0 == 2:
        v = torch.zeros(x0.shape[0], x0.shape[1], 2 * x0.shape[2], 2 * x0.shape[3], dtype=x0.dtype)
        v[:, :, ::2, ::2] = x0
    return v if x1 is None else torch.cat([v, x1], 1)


def dilated(w, dil):
    """the k x k kernel with dil - 1 zeros between its taps"""
    if dil <= 1:
        return w
    k = w.shape[-1]
    out = torch.zeros(w.shape[0], w.shape[1], (k - 1) * dil + 1, (k - 1) * dil + 1, dtype=w.dtype)
    out[:, :, ::dil, ::dil] = w
    return out


def pool2(v):
    """sum over 2 x 2 pixel blocks"""
    return v[:, :, 0::2, 0::2] + v[:, :, 0::2, 1::2] + v[:, :, 1::2, 0::2] + v[:, :, 1::2, 1::2]


def _cview(t):
    return None if t is None else t.double().view(1, -1, 1, 1)


def reference_and_bound(code, x0, x1, w, *, up0=0, stride=1, pad=0, dilation=1, scale=None, shift=None, residual=None, relu=0,
                        store_code=None, pool0=0):
    """(reference, bound) in float64, NCHW, of the launch's output before it is split: see the module docstring for every term"""
    src, wd = source(x0, x1, up0).double(), dilated(w.double(), dilation)
    val = F.conv2d(src, wd, stride=stride, padding=pad)
    kk = w[0].numel()
    err = gamma(kk if code == 0 else 2 * kk) * F.conv2d(src.abs(), wd.abs(), stride=stride, padding=pad)
    if pool0:
        mag, val, err = pool2(val.abs()), pool2(val), pool2(err)
        err = err + gamma(3) * (mag + err)
    if scale is not None:
        val, err = val * _cview(scale), err * _cview(scale).abs()
        err = err + U * (val.abs() + err)
    if shift is not None:
        val = val + _cview(shift)
        err = err + U * (val.abs() + err)
    if residual is not None:
        val = val + residual.double()
        err = err + U * (val.abs() + err)
    if relu:
        val = val.clamp_min(0)
    u, tiny = STORE[code if store_code is None else store_code]
    return val, err + (u * (val.abs() + err)).clamp_min(tiny)


@functools.lru_cache(maxsize=4)
def reference(case):
    """(reference, bound) of the case: channels of a split output side by side, the pooled form at half resolution"""
    x0, x1, w, scale, shift, res = inputs(case)
    return reference_and_bound(case.code, x0, x1, w, up0=case.up0, stride=case.stride, pad=case.pad, dilation=case.dilation, scale=scale,
                               shift=shift, residual=res, relu=case.relu, store_code=case.store_code, pool0=case.pool0)


def worst(err, bound):
    """max over the elements of err / bound; NaN (an unwritten element) stays NaN"""
    err, bound = err.double(), bound.double()
    if torch.isnan(err).any():
        return math.nan
    return (err / bound).max().item()


def figure_against(got, ref, bound):
    return worst((got.double() - ref).abs(), bound)


def figure(got, case):
    """max over the elements of |got - ref| / bound; got in NCHW on the CPU (a split output concatenated along channels)"""
    ref, bound = reference(case)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return figure_against(got, ref, bound)


def old_tolerance(case):
    """per element what hip_helpers.tol allowed: atol + rtol |ref| with atol scaled by max |ref|"""
    ref, _ = reference(case)
    t = tol(case.code, ref.abs().max().item())
    return t["atol"] + t["rtol"] * ref.abs()


# ---- fp32 on the CPU: an honest evaluation and the mutations the bound must catch -------------------------------------------------
def _conv32(case, src, w):
    return F.conv2d(src, dilated(w, case.dilation), stride=case.stride, padding=case.pad)


def _finish32(case, acc):
    """the epilogue in fp32 and the store's rounding"""
    _, _, _, scale, shift, res = inputs(case)
    v = pool2(acc) if case.pool0 else acc
    if scale is not None:
        v = v * scale.view(1, -1, 1, 1)
    if shift is not None:
        v = v + shift.view(1, -1, 1, 1)
    if res is not None:
        v = v + res
    if case.relu:
        v = v.clamp_min(0)
    return rounded(v, case.store_code)


def _taps(case):
    """(row, column) of the centre tap"""
    return case.k // 2, case.k // 2


def _last_stored(size, stuffed):
    """the last row / column of the virtual source that holds stored values (a zero-stuffed source ends on a row of zeros)"""
    return size - 2 if stuffed else size - 1


def cpu_fp32(case, mutation=None):
    """fp32 F.conv2d on the CPU with the fp32 epilogue, rounded to the stored type.  mutation:
    "chunks"   the accumulator is rounded to the storage type after every chunk of input channels;
    "channel"  one tap reads channel C-2 in place of C-1 in the last image column that holds stored values;
    "tail"     the last 8 channels (4 for fp32) of the centre tap are dropped on the last output row whose centre tap reads stored values."""
    x0, x1, w, *_ = inputs(case)
    src = source(x0, x1, case.up0)
    if mutation == "chunks":
        acc = None
        for c in range(0, case.cin, CHUNK[case.code]):
            part = _conv32(case, src[:, c:c + CHUNK[case.code]], w[:, c:c + CHUNK[case.code]])
            acc = rounded(part if acc is None else acc + part, case.code)
        return _finish32(case, acc)
    acc = _conv32(case, src, w)
    ch, cw = _taps(case)
    if mutation == "channel":
        col = _last_stored(case.w, case.up0 == 2)
        # a tap column kw that some output column reads at source column col: col = wo * stride - pad + kw * dilation
        kws = [kw for kw in (cw, case.k - 1, 0) if (col + case.pad - kw * case.dilation) % case.stride == 0 and
               0 <= (col + case.pad - kw * case.dilation) // case.stride < case.wout]
        dx = torch.zeros_like(src)
        dx[:, -1, :, col] = src[:, -2, :, col] - src[:, -1, :, col]
        wt = torch.zeros_like(w)
        wt[:, :, ch, kws[0]] = w[:, :, ch, kws[0]]
        acc = acc + _conv32(case, dx, wt)
    elif mutation == "tail":
        drop = 4 if case.code == 0 else 8
        rows = [ho for ho in range(case.hout) if not (case.up0 == 2 and (ho * case.stride) & 1)]      # (the centre tap of row ho reads source row ho * stride)
        wt = torch.zeros_like(w)
        wt[:, -drop:, ch, cw] = w[:, -drop:, ch, cw]
        acc = acc.clone()
        acc[:, :, rows[-1]] -= _conv32(case, src, wt)[:, :, rows[-1]]
    elif mutation is not None:
        raise ValueError(mutation)
    return _finish32(case, acc)


def independent_reference(case):
    """the float64 convolution once more, by another route: F.unfold (with its own dilation and stride) over the explicitly built
    source, one image at a time, and an einsum with the weights; then the float64 epilogue"""
    x0, x1, w, scale, shift, res = inputs(case)
    src, w64 = source(x0, x1, case.up0).double(), w.double().reshape(case.cout, -1)
    out = torch.empty(case.n, case.cout, case.hout, case.wout, dtype=torch.float64)
    for i in range(case.n):
        cols = F.unfold(src[i:i + 1], case.k, dilation=case.dilation, padding=case.pad, stride=case.stride)      # (1, cin k k, L)
        out[i] = torch.einsum("ok,kl->ol", w64, cols[0]).view(case.cout, case.hout, case.wout)
    if case.pool0:
        out = out.view(case.n, case.cout, case.hout // 2, 2, case.wout // 2, 2).sum((3, 5))
    if scale is not None:
        out = out * scale.double().view(1, -1, 1, 1)
    if shift is not None:
        out = out + shift.double().view(1, -1, 1, 1)
    if res is not None:
        out = out + res.double()
    return out.clamp_min(0) if case.relu else out
