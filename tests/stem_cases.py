"""What the stem tests share (tests/test_stem_host.py, tests/test_hip_stem_bounds.py and the stem assertions of tests/test_hip_ops.py):
the table of cases - one row per kernel form the launches of csrc/stem.hip can select (vs_stem_fwd, vs_stem_fwd_bins, vs_stem_wgrad), for
each dtype and option set that reaches it, with the launch structure (tiles, tiles per weight-gradient range, the shorter last range, the
slab-reduce group) written out by hand - seeded inputs, the float64 reference, the per-element bound with its derivation, and the figure
(measured error over bound) a test asserts to be at most 1.  U, gamma, STORE and worst are those of tests/conv_cases.py, reduce_depth
that of tests/wgrad_cases.py, and the seed scheme is theirs.

The stem is a 7 x 7 stride-2 pad-3 convolution of ONE fp32 input channel onto 64 channels.  The device always receives the fp32 image and
the fp32 weights.  The kernels on v_mfma_f32_16x16x32_bf16 (forms fwd-mfma16, fwd-bins, wgrad-mfma16: bf16 under option stem_bf16 1, the
default) round both to bf16 while they stage them, so their reference sees the rounded values; every other form (fp32, and the bf16-store
and fp16-store forms, which do fp32 arithmetic on the unrounded operands) is referred to the fp32 values themselves.  The gradient dy is
a value the storage type holds exactly.

Shapes (n, h, w), chosen against the 8 x 32 output tile (16 x 64 input pixels); every form runs all three:
  (3, 22, 70)    11 x 35 outputs: 2 x 2 tiles an image, the last row tile 3 rows high and the last column tile 3 columns wide, 12 tiles
  (2, 2, 2)      one output pixel an image, a patch that is nearly all padding, 2 tiles
  (1031, 4, 6)   2 x 3 outputs an image, 1031 tiles: seven workgroups of stem_fwd_bf16_kernel (grid min(tiles, 1024)) walk a second
                 tile; the fp32 weight gradient (cdiv(tiles, 1024) tiles a range) runs 516 ranges of 2, the last of 1; the bf16 one
                 (cdiv(tiles, 512)) 344 ranges of 3, the last of 2

The bound, per element.  U = 2^-24 is the unit roundoff of fp32, gamma_m = m U / (1 - m U) bounds m roundings in a row.  Every later term
is taken on the magnitude that flows through it: |value of the float64 reference at that point| + the error accumulated so far.

forward (vs_stem_fwd), S = conv(|x|, |w|) over the 49 taps:
  accumulation  fp32 (stem_fwd_kernel<T>: v_mfma_f32_16x16x4_f32 over k = 49 taps padded to 52): 13 MFMA steps of four chained fused
                multiply-adds, one rounding each - gamma_52 S.  The three padding taps multiply a zero weight and add exact zeros;
                charging them is sound.
                bf16 (stem_fwd_bf16_kernel: two steps of v_mfma_f32_16x16x32_bf16 over k = kh * 8 + kw): the products of the rounded
                operands are exact in fp32, how the instruction sums its 32 products is not documented, so each product is charged
                two roundings - gamma_{2 * 49} S, the convention of conv_cases.
  scale, shift  v * scale + shift: the error so far is multiplied by |scale|, one rounding each (a fused form rounds once).
  ReLU          exact and 1-Lipschitz: the bound carries over unchanged.
  store         half a unit in the last place of the stored type (STORE of conv_cases), never less than half its subnormal step.

weight gradient (vs_stem_wgrad), S = sum over the output pixels of |dy| * |x| in float64, m roundings on the way into dw - gamma_m S:
  accumulation  fp32 (stem_wgrad_kernel<T>): a wave's accumulator takes 64 MFMA steps of four fused multiply-adds for every tile of its
                range - 256 * tiles per range.
                bf16 (stem_wgrad_bf16_kernel): a wave takes two tile rows (two k-steps) a tile; the step in which a product enters
                is charged 32 roundings and every later one one - 32 + 2 * tiles per range - 1; then the four waves meet in LDS on
                wave 0 - 3.
  slab reduce   reduce_depth(group, ranges) of wgrad_cases: launch_slab_reduce sums the ranges' slabs, group by slab_reduce_groups'
                rule (64 * 49 floats: 1 below 8 ranges, 4 below 32, 16 from 32 on).
  store         dw is fp32: U (|ref| + the error so far), never less than 2^-150.

statistics bins (vs_stem_fwd_bins), per channel the totals bins.sum(0) / vs_stat_scale(k) against the float64 sum r and sum r^2 over the
valid output pixels of the float64 stem output r.  Per pixel the accumulator is within e = gamma_98 S of r.  A lane chains 4 adds for
every tile it walks (cdiv(tiles, 1024)), then 4 shuffle levels, then 3 adds across the waves: m = 4 * walk + 7, the squares one more.
Every workgroup that adds rounds its sum to a unit of the fixed-point scale (half a unit: 2^-25 for the sums, 2^-17 for the squares):
  sums      sum e + gamma_m sum (|r| + e) + workgroups * 2^-25
  squares   sum (2 |r| e + e^2) + gamma_{m+1} sum (|r| + e)^2 + workgroups * 2^-17
(the bound of test_conv_direct_kernel_statistics_rows_and_bins' bf16 branch).  The tensor z the bins launch stores must equal bit for bit
what vs_stem_fwd stores for the same operands without an epilogue.

There is no other absolute slack and no measured constant."""
import dataclasses
import functools

import torch
import torch.nn.functional as F

from conv_cases import DT, STORE, U, gamma, worst
from hip_helpers import option, rounded, tol
from wgrad_cases import reduce_depth

TPH, TPW = 8, 32                  # the output tile (csrc/stem.hip)
FWD_BLOCKS = 1024                 # stem_fwd_bf16_kernel: grid min(tiles, 1024)
WGRAD_BLOCKS = {"wgrad": 1024, "wgrad-mfma16": 512}      # kStemBlocks; the bf16 kernel's 512
DW = 64 * 49
NB = 16                           # stat_bins_rows(64)
FORMS = ("fwd", "fwd-mfma16", "fwd-bins", "wgrad", "wgrad-mfma16")
OFF, ON = (("stem_bf16", 0),), (("stem_bf16", 1),)


@dataclasses.dataclass(frozen=True)
class Shape:
    """tiles: 8 x 32 output tiles in all; (per, ranges, last): tiles per weight-gradient range, ranges and the tiles of the last range,
    for the fp32 kernel and for the bf16 MFMA kernel; group: the slab-reduce group of either"""
    n: int
    h: int
    w: int
    tiles: int
    walk: int                     # tiles the busiest workgroup of stem_fwd_bf16_kernel walks
    ranges32: tuple
    ranges16: tuple
    group32: int
    group16: int


SHAPES = (
    Shape(3, 22, 70, 12, 1, (1, 12, 1), (1, 12, 1), 4, 4),
    Shape(2, 2, 2, 2, 1, (1, 2, 1), (1, 2, 1), 1, 1),
    Shape(1031, 4, 6, 1031, 2, (2, 516, 1), (3, 344, 2), 16, 16),
)


@dataclasses.dataclass(frozen=True)
class Case:
    """form: the kernel the launch takes - "fwd" stem_fwd_kernel<T>, "fwd-mfma16" stem_fwd_bf16_kernel, "fwd-bins" the same with the
    statistics bins, "wgrad" stem_wgrad_kernel<T>, "wgrad-mfma16" stem_wgrad_bf16_kernel.  code: the dtype handed to the launch.
    refused: the launch must return non-zero and write nothing; ws_short: bytes withheld from the workspace; nb: bins rows."""
    label: str
    form: str
    code: int
    shape: Shape
    options: tuple = ()
    affine: int = 0
    relu: int = 0
    refused: bool = False
    ws_short: int = 0
    nb: int = NB

    @property
    def id(self):
        s = self.shape
        return f"{self.label}-{s.n}x{s.h}x{s.w}-{DT[self.code]}"

    @property
    def seed(self):
        return sum(ord(ch) * (i + 1) for i, ch in enumerate(self.id)) % 100003

    @property
    def mfma16(self):
        """the kernel rounds the image and the weights to bf16 while staging"""
        return self.form in ("fwd-mfma16", "fwd-bins", "wgrad-mfma16")

    @property
    def is_wgrad(self):
        return self.form.startswith("wgrad")

    @property
    def hout(self):
        return self.shape.h // 2

    @property
    def wout(self):
        return self.shape.w // 2

    @property
    def ranges(self):
        """(tiles per range, ranges, tiles of the last range) of a weight-gradient row"""
        return self.shape.ranges16 if self.form == "wgrad-mfma16" else self.shape.ranges32

    @property
    def group(self):
        return self.shape.group16 if self.form == "wgrad-mfma16" else self.shape.group32


# (form, dtype, options, label): the hand-written list of what the three launches can select
SELECT = [
    ("fwd", 0, (), "fwd"), ("fwd", 1, OFF, "fwd-bf16-store"), ("fwd", 2, (), "fwd-fp16-store"),
    ("fwd-mfma16", 1, ON, "fwd-mfma16"),
    ("fwd-bins", 1, ON, "fwd-bins"),
    ("wgrad", 0, (), "wgrad"), ("wgrad", 1, OFF, "wgrad-bf16-dy"),
    ("wgrad-mfma16", 1, ON, "wgrad-mfma16"),
]
EPILOGUES = (("", 0, 0), ("-affine+relu", 1, 1), ("-relu", 0, 1))


def _cases():
    out = []
    for form, code, opts, label in SELECT:
        for shape in SHAPES:
            for suffix, affine, relu in (EPILOGUES if form in ("fwd", "fwd-mfma16") else EPILOGUES[:1]):
                out.append(Case(label + suffix, form, code, shape, options=opts, affine=affine, relu=relu))
    return out


CASES = _cases()
_S = SHAPES[0]
_ODD_H, _ODD_W = Shape(3, 21, 70, 0, 0, (), (), 0, 0), Shape(3, 22, 69, 0, 0, (), (), 0, 0)      # no launch: no structure
REFUSED = [
    Case("refused-fp16-wgrad", "wgrad", 2, _S, refused=True),
    Case("refused-odd-h-fwd", "fwd", 0, _ODD_H, refused=True),
    Case("refused-odd-h-wgrad", "wgrad", 0, _ODD_H, refused=True),
    Case("refused-odd-h-bins", "fwd-bins", 1, _ODD_H, options=ON, refused=True),
    Case("refused-odd-w-fwd", "fwd", 0, _ODD_W, refused=True),
    Case("refused-odd-w-wgrad", "wgrad-mfma16", 1, _ODD_W, options=ON, refused=True),
    Case("refused-odd-w-bins", "fwd-bins", 1, _ODD_W, options=ON, refused=True),
    Case("refused-workspace-a-byte-short", "wgrad", 0, _S, refused=True, ws_short=1),
    Case("refused-workspace-a-byte-short", "wgrad-mfma16", 1, _S, options=ON, refused=True, ws_short=1),
    Case("refused-bins-fp32", "fwd-bins", 0, _S, options=ON, refused=True),
    Case("refused-bins-option-off", "fwd-bins", 1, _S, options=OFF, refused=True),
    Case("refused-bins-nb-12", "fwd-bins", 1, _S, options=ON, refused=True, nb=12),
]


# ---- the launch structure, from the constants above -------------------------------------------------------------------------------
def cdiv(a, b):
    return -(-a // b)


def tile_count(n, h, w):
    return n * cdiv(h // 2, TPH) * cdiv(w // 2, TPW)


def range_structure(tiles, blocks):
    """(tiles per range, ranges, tiles of the last range) of vs_stem_wgrad: per = cdiv(total, blocks), cdiv(total, per) ranges"""
    per = cdiv(tiles, blocks)
    ranges = cdiv(tiles, per)
    return per, ranges, tiles - (ranges - 1) * per


def slab_group(ranges):
    """slab_reduce_groups for 64 * 49 floats (784 float4, below both of its size thresholds) in aligned buffers"""
    assert DW % 4 == 0 and DW // 4 < 32768
    return 1 if ranges < 8 else 4 if ranges < 32 else 16


def tiles_of(case):
    """the tiles in the kernels' order (image, tile row, tile column) as (image, row slice, column slice) of the output"""
    return [(i, slice(ty * TPH, min(case.hout, (ty + 1) * TPH)), slice(tx * TPW, min(case.wout, (tx + 1) * TPW)))
            for i in range(case.shape.n) for ty in range(cdiv(case.hout, TPH)) for tx in range(cdiv(case.wout, TPW))]


def workgroups(case):
    """workgroups of stem_fwd_bf16_kernel, each of which adds once to the bins"""
    return min(case.shape.tiles, FWD_BLOCKS)


# ---- the launch of a case -----------------------------------------------------------------------------------------------------------
def out_elems(case):
    """elements of the tensor the launch writes (y / z in the row's dtype, dw in fp32)"""
    return DW if case.is_wgrad else case.shape.n * case.hout * case.wout * 64


def launch(L, case, x, w, out, *, scale=None, shift=None, dy=None, ws=None, ws_bytes=0, bins=None, stream=None):
    """the row's launch through the C ABI under the row's options; the tensors live wherever the caller put them (a refused launch
    dereferences none of them, so the host tests hand it CPU tensors).  Returns the status."""
    s = case.shape
    with option(**dict(case.options)):
        if case.form == "fwd-bins":
            return L.lib.vs_stem_fwd_bins(case.code, L.ptr(x), L.ptr(w), L.ptr(out), s.n, s.h, s.w, L.ptr(bins), case.nb, stream)
        if case.is_wgrad:
            return L.lib.vs_stem_wgrad(case.code, L.ptr(x), L.ptr(dy), L.ptr(out), L.ptr(ws), ws_bytes, s.n, s.h, s.w, stream)
        return L.lib.vs_stem_fwd(case.code, L.ptr(x), L.ptr(w), L.ptr(scale), L.ptr(shift), case.relu, L.ptr(out), s.n, s.h, s.w, stream)


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=8)
def inputs(case):
    """x (n, 1, h, w), w (64, 1, 7, 7), scale, shift (or None), dy (n, 64, h / 2, w / 2; the weight-gradient rows only) - fp32 CPU tensors
    as the device receives them: image and weights unrounded, dy a value the storage type holds exactly"""
    s = case.shape
    g = torch.Generator().manual_seed(case.seed)
    x = torch.randn(s.n, 1, s.h, s.w, generator=g)
    w = torch.randn(64, 1, 7, 7, generator=g) / 7.0
    scale = torch.rand(64, generator=g) + 0.5 if case.affine else None
    shift = torch.randn(64, generator=g) if case.affine else None
    dy = rounded(torch.randn(s.n, 64, s.h // 2, s.w // 2, generator=g), 1 if case.code == 2 else case.code) if case.is_wgrad else None
    return x, w, scale, shift, dy


def seen(case):
    """(x, w) as the kernel's arithmetic sees them: rounded to bf16 by the MFMA-16 forms, the fp32 values otherwise"""
    x, w, *_ = inputs(case)
    return (rounded(x, 1), rounded(w, 1)) if case.mfma16 else (x, w)


# ---- references and bounds ----------------------------------------------------------------------------------------------------------
def _conv(x, w):
    return F.conv2d(x, w, stride=2, padding=3)


def _cview(t):
    return t.double().view(1, -1, 1, 1)


def fwd_reference_and_bound(x, w, mfma16, store_code, scale=None, shift=None, relu=0):
    """(reference, bound) in float64, NCHW, for operands as the arithmetic sees them: see the module docstring for every term"""
    val = _conv(x.double(), w.double())
    err = gamma(2 * 49 if mfma16 else 52) * _conv(x.double().abs(), w.double().abs())
    if scale is not None:
        val, err = val * _cview(scale), err * _cview(scale).abs()
        err = err + U * (val.abs() + err)
        val = val + _cview(shift)
        err = err + U * (val.abs() + err)
    if relu:
        val = val.clamp_min(0)
    u, tiny = STORE[store_code]
    return val, err + (u * (val.abs() + err)).clamp_min(tiny)


def _wgrad(x, dy):
    """d sum(conv(x, w) * dy) / dw as (64, 49)"""
    w = torch.zeros(64, 1, 7, 7, dtype=x.dtype).requires_grad_()
    (_conv(x, w) * dy).sum().backward()
    return w.grad.reshape(64, 49)


def wgrad_roundings(mfma16, per, ranges, group):
    chain = 32 + 2 * per - 1 + 3 if mfma16 else 256 * per
    return chain + reduce_depth(group, ranges)


def wgrad_reference_and_bound(x, dy, mfma16, per, ranges, group):
    """(reference, bound) in float64 as (64, 49), for the image as the arithmetic sees it"""
    ref = _wgrad(x.double(), dy.double())
    err = gamma(wgrad_roundings(mfma16, per, ranges, group)) * _wgrad(x.double().abs(), dy.double().abs())
    return ref, err + (U * (ref.abs() + err)).clamp_min(2.0 ** -150)


def bins_reference_and_bound(x, w, walk, wgs):
    """(reference, bound) as (2, 64): the sums and the sums of squares over the valid output pixels, for operands rounded to bf16"""
    r = _conv(x.double(), w.double())
    e = gamma(2 * 49) * _conv(x.double().abs(), w.double().abs())
    mag = r.abs() + e
    m = 4 * walk + 4 + 3
    dims = (0, 2, 3)
    b1 = e.sum(dims) + gamma(m) * mag.sum(dims) + wgs * 2.0 ** -25
    b2 = (2 * r.abs() * e + e * e).sum(dims) + gamma(m + 1) * (mag * mag).sum(dims) + wgs * 2.0 ** -17
    return torch.stack([r.sum(dims), (r * r).sum(dims)]), torch.stack([b1, b2])


@functools.lru_cache(maxsize=8)
def reference(case):
    """(reference, bound) of the row in float64: NCHW (forward), (64, 49) (weight gradient), (2, 64) (bins)"""
    x, w = seen(case)
    _, _, scale, shift, dy = inputs(case)
    if case.form == "fwd-bins":
        return bins_reference_and_bound(x, w, case.shape.walk, workgroups(case))
    if case.is_wgrad:
        per, ranges, _ = case.ranges
        return wgrad_reference_and_bound(x, dy, case.mfma16, per, ranges, case.group)
    return fwd_reference_and_bound(x, w, case.mfma16, case.code, scale, shift, case.relu)


def stored_reference(case):
    """(reference, bound) of the tensor z a bins row stores: the forward of the same operands without an epilogue"""
    x, w = seen(case)
    return fwd_reference_and_bound(x, w, True, case.code)


def figure_against(got, ref, bound):
    return worst((got.double() - ref).abs(), bound)


def figure(got, case):
    """max over the elements of |got - ref| / bound; got on the CPU laid out as the reference (forward: NCHW)"""
    ref, bound = reference(case)
    assert tuple(got.shape) == tuple(ref.shape), (got.shape, ref.shape)
    return figure_against(got, ref, bound)


def bins_totals(bins, scales):
    """[nb][2][64] int64 bins -> (2, 64) float64 totals; scales = (vs_stat_scale(0), vs_stat_scale(1))"""
    tot = bins.sum(0).double()
    return torch.stack([tot[0] / scales[0], tot[1] / scales[1]])


def old_tolerance(case):
    """per element what the assertions of test_stem_fwd_and_wgrad allow: hip_helpers.tol with atol scaled by max |ref| (forward), rtol 1e-3
    and atol 1e-3 max |ref| (weight gradient)"""
    ref, _ = reference(case)
    if case.is_wgrad:
        return 1e-3 * ref.abs().max() + 1e-3 * ref.abs()
    t = tol(case.code, ref.abs().max().item())
    return t["atol"] + t["rtol"] * ref.abs()


def independent_reference(case):
    """the float64 result once more by another route: F.unfold of the explicitly zero-padded image, one image at a time, and an einsum
    with the weights (forward, bins) or with the gradient over the pixels (weight gradient); then the float64 epilogue"""
    x, w = seen(case)
    _, _, scale, shift, dy = inputs(case)
    s = case.shape
    xp = F.pad(x.double(), (3, 3, 3, 3))
    w64 = w.double().reshape(64, 49)
    out = torch.zeros(64, 49, dtype=torch.float64) if case.is_wgrad else torch.empty(s.n, 64, case.hout, case.wout, dtype=torch.float64)
    for i in range(s.n):
        cols = F.unfold(xp[i:i + 1], 7, stride=2)[0]                       # (49, L)
        if case.is_wgrad:
            out += torch.einsum("ol,kl->ok", dy[i].double().reshape(64, -1), cols)
        else:
            out[i] = torch.einsum("ok,kl->ol", w64, cols).view(64, case.hout, case.wout)
    if case.is_wgrad:
        return out
    if case.form == "fwd-bins":
        return torch.stack([out.sum((0, 2, 3)), (out * out).sum((0, 2, 3))])
    if scale is not None:
        out = out * _cview(scale) + _cview(shift)
    return out.clamp_min(0) if case.relu else out


# ---- fp32 on the CPU: an honest evaluation and the mutations the bound must catch -----------------------------------------------------
MUTATIONS = ("padding", "tile", "ragged", "slab")


def applies(mutation, case):
    """padding: every row; tile: every row (a forward row leaves the tile unwritten); ragged: the bins rows; slab: the weight gradients"""
    return {"padding": True, "tile": True, "ragged": case.form == "fwd-bins", "slab": case.is_wgrad}[mutation]


def _padded(x, mutation):
    """the image with its three columns / rows of zero padding written out; "padding": the column left of the image (input column -1)
    holds the image's first column instead of zeros"""
    xp = F.pad(x, (3, 3, 3, 3))
    if mutation == "padding":
        xp[:, :, 3:-3, 2] = x[:, :, :, 0]
    return xp


def _masked(dy, tiles):
    out = torch.zeros_like(dy)
    for i, rs, cs in tiles:
        out[i, :, rs, cs] = dy[i, :, rs, cs]
    return out


def cpu_fp32(case, mutation=None):
    """the row's result in fp32 torch on the CPU (operands rounded to bf16 first where the kernel rounds them), with the fp32 epilogue and
    the store's rounding; laid out as reference(case).  mutation:
    "padding"  one padding column is read as data: input column -1 holds the image's column 0;
    "tile"     one tile of a walk is dropped - forward: the last tile is left unwritten (NaN); weight gradient: the last tile of the
               first range is not accumulated; bins: the last tile a workgroup walks is not counted;
    "ragged"   one pixel of a ragged tile - the one right of the first image's first row - is counted into the bins;
    "slab"     the last range's slab is left out of the reduce."""
    assert mutation is None or (mutation in MUTATIONS and applies(mutation, case)), mutation
    x, w = seen(case)
    _, _, scale, shift, dy = inputs(case)
    xp = _padded(x, mutation)
    if case.is_wgrad:
        wz = torch.zeros(64, 1, 7, 7).requires_grad_()
        (F.conv2d(xp, wz, stride=2) * dy).sum().backward()
        dw = wz.grad.reshape(64, 49)
        if mutation in ("tile", "slab"):
            per = case.ranges[0]
            tiles = tiles_of(case)
            gone = tiles[per - 1:per] if mutation == "tile" else tiles[(case.ranges[1] - 1) * per:]
            dw = dw - _wgrad(x, _masked(dy, gone))
        return dw
    acc = F.conv2d(xp, w, stride=2)
    if case.form == "fwd-bins":
        v = acc
        if mutation == "tile":
            v = acc.clone()
            i, rs, cs = tiles_of(case)[-1]
            v[i, :, rs, cs] = 0
        s1, s2 = v.sum((0, 2, 3)), (v * v).sum((0, 2, 3))
        if mutation == "ragged":
            extra = F.conv2d(F.pad(x, (3, 5, 3, 3)), w, stride=2)[0, :, 0, case.wout]      # the output column right of the image's edge
            s1, s2 = s1 + extra, s2 + extra * extra
        return torch.stack([torch.round(s1.double() * 2.0 ** 24) / 2.0 ** 24, torch.round(s2.double() * 2.0 ** 16) / 2.0 ** 16])
    v = acc
    if scale is not None:
        v = v * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    if case.relu:
        v = v.clamp_min(0)
    v = rounded(v, case.code)
    if mutation == "tile":
        i, rs, cs = tiles_of(case)[-1]
        v[i, :, rs, cs] = float("nan")
    return v
