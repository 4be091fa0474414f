"""What the weight-gradient tests share (tests/test_wgrad_host.py, tests/test_hip_wgrad_bounds.py, and the weight-gradient assertions of
tests/test_hip_ops.py and tests/test_hip_ring_kernels.py): the table of cases - one row per kernel instantiation the launch of
csrc/conv_wgrad.hip can select (vs_conv2d_wgrad, vs_head_wgrad_planes), for each dtype it is built for, with the plan structure
(vs_wgrad_plan) written out by hand - seeded inputs, the float64 reference, the per-element bound with its derivation, and the figure
(measured error over bound) a test asserts to be at most 1.  The helpers source, dilated, gamma, worst and rounded and the seed scheme
are those of tests/conv_cases.py.

Covered: the generic kernel (fp32, and bf16 where cout is no multiple of 8), the bf16 fast kernel, the ring kernel in its four forms,
the three row-streaming kernels at their three widths, the four slab-reduce kernels and the grouped extract; with the loader forms
(nearest x2 + concatenation, dilation 2 / 4, both stride-2 tile shapes), the split structure (one split, two tiles per split, a
shorter last split, the three workgroup assignment modes, every reduce group) and the launches that must be refused.  The stem's
weight gradient (csrc/stem.hip) has its own table of this kind, tests/stem_cases.py.  Not covered here: the depthwise weight gradients,
which keep their own tests.

The bound, per element of dw.  U = 2^-24 is the unit roundoff of fp32, gamma_m = m U / (1 - m U) bounds m roundings in a row.  The
inputs are fp32 values the storage type holds exactly and every product of two of them is exact in fp32 (16-bit operands) or rounded
once inside the fused multiply-add (fp32), so the error is that of summing K = n * hout * wout products in fp32, and a sum in which no
term meets more than m roundings on its way into the result is within gamma_m * S of the exact one, S = sum over the pixels of
|dy| * |x| in float64.  m is read off the code of the family and depends on the row's plan (tiles per split, splits, reduce group):

  accumulation  A wave's accumulator is one chain of MFMA steps, `steps` = tiles per split * k-steps per tile / K-waves long (the
                k-steps of a tile are dealt to the K-waves round-robin; the last split's chain is shorter).
                fp32 (v_mfma_f32_16x16x4_f32): a step is four fused multiply-adds in k order, one rounding each - 4 * steps.
                bf16 (v_mfma_f32_16x16x32_bf16): how the instruction sums its 32 exact products is not documented, so the step in
                which a product enters is charged KSTEP = 32 roundings (any order over the 32 products and the accumulator), and every
                later step of the chain one (the accumulator joins that step's sum) - 32 + steps - 1.
                  generic kernel  k-steps per tile = 64 pt / KSTEP, K-waves WK = 4 / wo
                  fast kernel     k-steps per tile = 2 pt, K-groups: 2 for 1x1 kernels, 1 for 3x3 (the waves split the taps)
                  ring kernel     4 k-steps per 128-pixel tile, no K split inside the workgroup
                  row kernels     a row step is wq k-steps per wave (32 channels behind the upsampling: a source row feeds two gradient
                                  rows and a tap's accumulator takes up to two MFMAs per k-step - 2 wq)
  combine       the K-waves meet in LDS, summed in wave order onto wave 0: WK - 1 roundings (generic), 1 (fast 1x1), 3 (row kernels).
  slab reduce   lane group g of G sums slabs g, g + G, .. alternately into two accumulators (ceil(c / 2) adds for c = ceil(nsplit / G)
                slabs), adds the two (1) and the groups meet in LDS in order (G - 1); the scalar kernel (group 0: a tensor that is no
                multiple of four floats or a buffer off 16-byte alignment) has four lane groups and a two-level tree (2).  A sum of nsplit
                slabs has nsplit - 1 adds in all: never more than that.
  store         dw is fp32: nothing is rounded again; U (|ref| + the error so far) is charged all the same, never less than 2^-150, half
                the smallest subnormal step - the one absolute term, a property of the format.
There is no other absolute slack and no measured constant.  The order-free alternative - gamma_2K * S, any summation order over all K
products with two roundings each - is 33 times looser in the median over this table (1.25 times for the smallest fp32 row, whose one
chain covers nearly all of K; 70 times for a bf16 row of K about 2 000 and m about 60; thousands of times for the 99 000-pixel rows) and
is not used: it grows with K while the chains the kernels run do not, and |dw| itself grows with sqrt(K) only."""
import dataclasses
import functools

import torch
import torch.nn.functional as F

from conv_cases import DT, U, dilated, gamma, source, worst
from hip_helpers import conv_desc, option, rounded

GENERIC, FAST, RING, ROWS = 0, 1, 2, 3
FAMILY = {GENERIC: "generic", FAST: "fast", RING: "ring", ROWS: "rows"}
KSTEP = {0: 4, 1: 32}
CHUNK = {0: 16, 1: 32}          # input channels per workgroup (conv_wgrad.hip: WT<T>::CK)
PLAN_FIELDS = ("family", "wo", "taps", "stride", "pt", "dil", "imgs", "rows_form", "wq", "nsplit", "tiles_per_split", "xmode", "ppx",
               "reduce_group", "extract", "workspace_bytes")


@dataclasses.dataclass(frozen=True)
class Plan:
    """vs_wgrad_plan, field for field"""
    family: int
    wo: int
    taps: int
    stride: int
    pt: int
    dil: int
    imgs: int
    rows_form: int
    wq: int
    nsplit: int
    tiles_per_split: int
    xmode: int
    ppx: int
    reduce_group: int
    extract: int
    workspace_bytes: int


def tiled(family, wo, taps, stride, pt, dil, nsplit, per, ws, *, xmode=0, ppx=0, red=None, extract=0, imgs=0):
    """a row's plan on the tiled kernels; red: the slab-reduce group of an aligned launch, None = one split, no reduce"""
    assert (red is None) == (nsplit == 1)
    return Plan(family, wo, taps, stride, pt, dil, imgs, 0, 0, nsplit, per, xmode, ppx, -1 if red is None else red, extract, ws)


def rows_plan(form, wq, nsplit, per, red, ws):
    return Plan(ROWS, 1, 9, 1, 0, 1, 0, form, wq, nsplit, per, 0, 0, red, 0, ws)


# ---- the table ------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Case:
    """h, w: the virtual input (after the loader's x2); pad = dilation * (k // 2).  inst: which instantiation the row stands for -
    (family, wo, taps, stride, pt, dilation) of conv_wgrad_kernel / conv_wgrad_bf16_kernel, ("ring", mo, imgs), ("rows", form, wq); None
    for the rows that run a loader form, a split structure or the grouped path on an instantiation another row already stands for.
    classes > 0: the head's planes launch (vs_head_wgrad_planes) - dy is fp32 NCHW planes of `classes` channels, dw [classes][9][16].
    ws_shift: floats the workspace pointer is moved off 16-byte alignment (the launch then takes the scalar slab reduce, group 0, where
    the query, which assumes aligned buffers, answers the plan's reduce_group).  refused: the launch and the query must return non-zero;
    ws_short: bytes withheld from the workspace (the query still answers the plan)."""
    label: str
    code: int                    # 0 = fp32, 1 = bf16, 2 = fp16 (refused)
    n: int
    h: int
    w: int
    c0: int
    cout: int
    plan: Plan = None
    k: int = 3
    stride: int = 1
    dilation: int = 1
    c1: int = 0
    up0: int = 0
    cg: int = 0                  # channels per group of a grouped layer (c0 == cout)
    classes: int = 0
    options: tuple = ()
    inst: tuple = None
    ws_shift: int = 0
    refused: bool = False
    ws_short: int = 0

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
    def family(self):
        return FAMILY[self.plan.family]

    @property
    def dw_shape(self):
        """the layout the launch writes"""
        if self.classes:
            return (self.classes, 9, 16)
        return (self.cout, self.k * self.k, self.cg or self.cin)

    @property
    def reduce_group(self):
        """the slab reduce the launch takes: the plan's, or the scalar kernel where the workspace is moved off alignment"""
        return 0 if self.ws_shift and self.plan.nsplit > 1 else self.plan.reduce_group


def _opts(target, xcd=0, slab_mb=0, ring=1):
    """no slab budget (wgrad_slab_mb 0): the launch asks for cdiv(target, cout tiles * cin chunks) splits, at most one per tile"""
    return (("wgrad_xcd", xcd), ("wgrad_slab_mb", slab_mb), ("wgrad_target_plain", target), ("wgrad_target", target), ("wgrad_ring", ring))


WG = _opts(16)


def _ws(nsplit, cout, taps, cin, extra=0):
    return (nsplit + extra) * cout * taps * cin * 4


# The generic and the fast kernel: (taps, stride, pt) x the three cout widths.  c0 = 40: 32 + 8 for bf16, 16 + 16 + 8 for fp32.  Tiles:
# 16 x 8 pixels (pt 2), 8 x 8 (pt 1; stride 2: 16 x 4 from 16 output columns on).  Two cout tiles and three (fp32) / two (bf16) cin chunks
# a row: 6 / 4 (cout tile, cin chunk) pairs, so WG asks for 3 / 4 splits.
#   (taps, stride, pt): (n, h, w), tiles, {pairs: (nsplit, tiles per split)}
TILE_FORMS = {
    (9, 1, 2): ((3, 20, 36), 27, {6: (3, 9), 4: (4, 7)}),
    (1, 1, 2): ((3, 20, 36), 27, {6: (3, 9), 4: (4, 7)}),
    (9, 1, 1): ((3, 20, 12), 18, {6: (3, 6), 4: (4, 5)}),
    (1, 1, 1): ((3, 7, 9), 6, {6: (3, 2), 4: (3, 2)}),
    (9, 2, 1): ((3, 19, 23), 12, {6: (3, 4), 4: (4, 3)}),
    (1, 2, 1): ((3, 19, 23), 12, {6: (3, 4), 4: (4, 3)}),
}
# the dilated 3x3 forms: (dilation, pt): (n, h, w), tiles, {pairs: (nsplit, tiles per split)}; wo 4 and 2 only
DILATED_FORMS = {
    (2, 2): ((3, 20, 36), 27, {6: (3, 9), 4: (4, 7)}),
    (2, 1): ((3, 20, 12), 18, {6: (3, 6), 4: (4, 5)}),
    (4, 1): ((3, 20, 12), 18, {6: (3, 6), 4: (4, 5)}),
}
COUT = {0: {4: 72, 2: 40, 1: 24}, FAST: {4: 72, 2: 40, 1: 24}, "generic-bf16": {4: 68, 2: 36, 1: 20}}


def _instantiation_cases():
    out = []
    for family, code in ((GENERIC, 0), (GENERIC, 1), (FAST, 1)):
        couts = COUT["generic-bf16"] if (family, code) == (GENERIC, 1) else COUT[family]
        pairs = 6 if code == 0 else 4
        red = 1                                       # fewer than 8 slabs: one lane group
        for wo in (4, 2, 1):
            cout = couts[wo]
            for (taps, stride, pt), ((n, h, w), _, split) in TILE_FORMS.items():
                nsplit, per = split[pairs]
                if (family, code, wo, pt) == (GENERIC, 1, 1, 1):
                    # two k-steps a tile cannot feed the four K-waves of a 16-cout workgroup: geom() keeps the width and does not split
                    nsplit, per = 1, {(9, 1): 18, (1, 1): 6, (9, 2): 12, (1, 2): 12}[taps, stride]
                k = 3 if taps == 9 else 1
                plan = tiled(family, wo, taps, stride, pt, 1, nsplit, per, _ws(nsplit, cout, taps, 40), red=None if nsplit == 1 else red)
                out.append(Case(f"{FAMILY[family]}{wo}-k{k}s{stride}pt{pt}-{n}x{h}x{w}x40to{cout}", code, n, h, w, 40, cout, plan, k=k, stride=stride,
                                options=WG, inst=(family, wo, taps, stride, pt, 1)))
        for wo in (4, 2):
            cout = couts[wo]
            for (dil, pt), ((n, h, w), _, split) in DILATED_FORMS.items():
                nsplit, per = split[pairs]
                plan = tiled(family, wo, 9, 1, pt, dil, nsplit, per, _ws(nsplit, cout, 9, 40), red=red)
                out.append(Case(f"{FAMILY[family]}{wo}-k3d{dil}pt{pt}-{n}x{h}x{w}x40to{cout}", code, n, h, w, 40, cout, plan, dilation=dil,
                                options=WG, inst=(family, wo, 9, 1, pt, dil)))
    return out


# The ring kernel (bf16, stride-1 3x3, channel counts in whole chunks of 32): 16 x 8 tiles at the three cout widths, and two 8 x 8 images
# per tile.  3 x 20 x 36: 27 tiles, 4 pairs -> 4 splits of 7; 8 x 8 x 8: 4 tiles, target 8 -> 2 splits of 2.
RING_CASES = [
    Case("ring4-3x20x36x32+32to72", 1, 3, 20, 36, 32, 72, tiled(RING, 4, 9, 1, 2, 1, 4, 7, _ws(4, 72, 9, 64), red=1, imgs=1), c1=32, options=WG, inst=("ring", 4, 1)),
    Case("ring2-3x20x36x32+32to40", 1, 3, 20, 36, 32, 40, tiled(RING, 2, 9, 1, 2, 1, 4, 7, _ws(4, 40, 9, 64), red=1, imgs=1), c1=32, options=WG, inst=("ring", 2, 1)),
    Case("ring1-3x20x36x32+32to24", 1, 3, 20, 36, 32, 24, tiled(RING, 1, 9, 1, 2, 1, 4, 7, _ws(4, 24, 9, 64), red=1, imgs=1), c1=32, options=WG, inst=("ring", 1, 1)),
    Case("ring4-two-images-8x8x8x64to72", 1, 8, 8, 8, 64, 72, tiled(RING, 4, 9, 1, 2, 1, 2, 2, _ws(2, 72, 9, 64), red=1, imgs=2), options=_opts(8), inst=("ring", 4, 2)),
]

# The loader forms: nearest x2 + concatenation on the generic (fp32, bf16), fast and ring kernels (c0 a whole number of chunks, the
# partner ragged where the kernel takes ragged channel counts); the 16 x 4 tiles of a stride-2 layer with 16 output columns or more
# (2 x 24 x 40 -> 12 x 20: 3 x 2 tiles an image).  72 input channels: 5 chunks in fp32 (10 pairs: 2 splits of 14), 3 in bf16 (6 pairs: 3 of 9).
FORM_CASES = [
    Case("generic4-up1+concat-3x20x36x32+40to72", 0, 3, 20, 36, 32, 72, tiled(GENERIC, 4, 9, 1, 2, 1, 2, 14, _ws(2, 72, 9, 72), red=1), c1=40, up0=1, options=WG),
    Case("generic4-up1+concat-3x20x36x32+40to68", 1, 3, 20, 36, 32, 68, tiled(GENERIC, 4, 9, 1, 2, 1, 3, 9, _ws(3, 68, 9, 72), red=1), c1=40, up0=1, options=WG),
    Case("fast4-up1+concat-3x20x36x32+40to72", 1, 3, 20, 36, 32, 72, tiled(FAST, 4, 9, 1, 2, 1, 3, 9, _ws(3, 72, 9, 72), red=1), c1=40, up0=1, options=WG),
    Case("ring4-up1+concat-3x20x36x32+32to72", 1, 3, 20, 36, 32, 72, tiled(RING, 4, 9, 1, 2, 1, 4, 7, _ws(4, 72, 9, 64), red=1, imgs=1), c1=32, up0=1, options=WG),
    Case("generic4-k3s2-16x4-2x24x40x40to72", 0, 2, 24, 40, 40, 72, tiled(GENERIC, 4, 9, 2, 1, 1, 3, 4, _ws(3, 72, 9, 40), red=1), stride=2, options=WG),
    Case("fast4-k3s2-16x4-2x24x40x40to72", 1, 2, 24, 40, 40, 72, tiled(FAST, 4, 9, 2, 1, 1, 4, 3, _ws(4, 72, 9, 40), red=1), stride=2, options=WG),
]


# Grouped layers (c0 == cout = 64: two 32-channel super-groups = two cout tiles of wo 2; one cin chunk in bf16, two in fp32): 4 / 8 / 16
# channels per group go through one more slab and the extract, 32 do not.  3 x 20 x 12: 18 tiles; 3 x 19 x 23 at stride 2: 12 tiles.
def _grouped_cases():
    out = []
    for code, family, (ns1, per1), (ns2, per2) in ((0, GENERIC, (4, 5), (4, 3)), (1, FAST, (6, 3), (6, 2))):
        for cg in (4, 8, 16, 32):
            ex = 1 if cg < 32 else 0
            out.append(Case(f"grouped{cg}-k3s1-3x20x12x64", code, 3, 20, 12, 64, 64, cg=cg, options=WG,
                            plan=tiled(family, 2, 9, 1, 1, 1, ns1, per1, _ws(ns1, 64, 9, 32, ex), red=1, extract=ex)))
            out.append(Case(f"grouped{cg}-k3s2-3x19x23x64", code, 3, 19, 23, 64, 64, cg=cg, stride=2, options=WG,
                            plan=tiled(family, 2, 9, 2, 1, 1, ns2, per2, _ws(ns2, 64, 9, 32, ex), red=1, extract=ex)))
    return out


# The row-streaming kernels (bf16, 16 couts, rows 128 / 256 / 512 wide): 16 plain channels, 32 channels behind the nearest upsampling,
# and the head's gradient planes.  A workgroup walks max(2, cdiv(steps, 256)) row steps; 3 x 5 rows = 15 steps -> 8 ranges of 2 (the last
# of 1) that cross the image boundaries; 3 x 6 upsampled rows = 9 source rows -> 5 ranges.  7 x 111 = 777 steps -> 195 ranges of 4: more
# steps a workgroup than the 3 in flight.  Slabs: 16 x 9 x 16 (plain), 16 x 9 x 32 (upsampled), classes x 9 x 16 (planes: the workspace is
# asked for as if all 16 gradient channels were live).
def _rows_cases():
    out = []
    for wq in (1, 2, 4):
        w = 128 * wq
        out.append(Case(f"rows16-3x5x{w}x16to16", 1, 3, 5, w, 16, 16, rows_plan(1, wq, 8, 2, 4, 8 * 2304 * 4), inst=("rows", 1, wq)))
        out.append(Case(f"rows-up32-3x6x{w}x32to16", 1, 3, 6, w, 32, 16, rows_plan(2, wq, 5, 2, 1, 5 * 4608 * 4), up0=1, inst=("rows", 2, wq)))
    for w, classes, inst in ((128, 1, None), (128, 2, ("rows", 3, 1)), (128, 4, None), (128, 7, None), (256, 4, ("rows", 3, 2)), (512, 7, ("rows", 3, 4))):
        out.append(Case(f"rows-planes{classes}-3x5x{w}x16", 1, 3, 5, w, 16, 16, rows_plan(3, w // 128, 8, 2, 4, 8 * 2304 * 4), classes=classes, inst=inst))
    out.append(Case("rows16-long-7x111x128x16to16", 1, 7, 111, 128, 16, 16, rows_plan(1, 1, 195, 4, 16, 195 * 2304 * 4)))
    out.append(Case("rows-up32-long-7x222x128x32to16", 1, 7, 222, 128, 32, 16, rows_plan(2, 1, 195, 4, 16, 195 * 4608 * 4), up0=1))
    out.append(Case("rows-planes2-long-7x111x128x16", 1, 7, 111, 128, 16, 16, rows_plan(3, 1, 195, 4, 16, 195 * 2304 * 4), classes=2))
    return out


# The split structure, through options alone, on a fast row (3 x 20 x 36 x 40 -> 72: 27 tiles, 4 pairs), a generic row (fp32,
# 3 x 20 x 12 x 40 -> 72: 18 tiles, 6 pairs) and a ring row (3 x 20 x 36 x 32 + 32 -> 72: 27 tiles, 4 pairs): one split (the launch writes
# dw itself), two tiles per split (the last split one), and - the instantiation rows have three or more tiles a split with a shorter last
# one - the workgroup assignment modes (wgrad_xcd: 1 = whole splits per XCD from 8 splits on, 2 = 1 / 2 / 4 splits over 8 / 4 / 2 XCDs
# with ppx pairs each) and every slab-reduce group: 1 below 8 slabs, 4 below 32, 16 from 32 on (n + 1 images: 36 / 24 tiles), 0 with the
# workspace moved off 16-byte alignment.
def _split_cases():
    out = []
    # (name, family, dtype, (h, w), pt, input channels, keywords of the case, keywords of the plan, images of the reduce16 row)
    for name, family, code, (h, w), pt, cin, kw, extra, many in (
            ("fast4", FAST, 1, (20, 36), 2, 40, dict(), dict(), 4),
            ("ring4", RING, 1, (20, 36), 2, 64, dict(c1=32), dict(imgs=1), 4),
            ("generic4", GENERIC, 0, (20, 12), 1, 40, dict(), dict(), 6)):
        c0 = cin - kw.get("c1", 0)

        def row(label, n, nsplit, per, options, red, ws_shift=0, **xcd):
            plan = tiled(family, 4, 9, 1, pt, 1, nsplit, per, _ws(nsplit, 72, 9, cin), red=red, **extra, **xcd)
            return Case(f"{name}-{label}-{n}x{h}x{w}x{cin}to72", code, n, h, w, c0, 72, plan, options=options, ws_shift=ws_shift, **kw)
        if family == GENERIC:      # 18 tiles, 6 pairs
            out.append(row("one-split", 3, 1, 18, _opts(1), None))
            out.append(row("two-tiles-a-split", 3, 9, 2, _opts(54), 4))
            out.append(row("reduce0-off-alignment", 3, 9, 2, _opts(54), 4, ws_shift=1))
            out.append(row("reduce16", many, 36, 1, _opts(216), 16))
            continue
        out.append(row("one-split", 3, 1, 27, _opts(1), None))      # 27 tiles, 4 pairs
        out.append(row("two-tiles-a-split", 3, 14, 2, _opts(56), 4))
        out.append(row("reduce0-off-alignment", 3, 14, 2, _opts(56), 4, ws_shift=1))
        out.append(row("reduce16", many, 36, 1, _opts(144), 16))
        out.append(row("xcd-whole-splits", 3, 14, 2, _opts(56, xcd=1), 4, xmode=1))
        out.append(row("xcd-4-splits", 3, 4, 7, _opts(16, xcd=1), 1, xmode=2, ppx=2))
        out.append(row("xcd-2-splits", 3, 2, 14, _opts(8, xcd=1), 1, xmode=2, ppx=1))
        out.append(row("xcd-one-split", 3, 1, 27, _opts(1, xcd=1), None, xmode=2, ppx=1))
    return out


CASES = _instantiation_cases() + RING_CASES + FORM_CASES + _grouped_cases() + _rows_cases() + _split_cases()

# Launches that must be refused: non-zero status from the query and from the launch, vs_last_error set, dw and the workspace untouched.
REFUSED = [
    Case("refused-stuffed-source-3x20x36x40to72", 1, 3, 20, 36, 40, 72, up0=2, options=WG, refused=True),
    Case("refused-stuffed-source-3x20x36x40to72", 0, 3, 20, 36, 40, 72, up0=2, options=WG, refused=True),
    Case("refused-fp16-3x20x36x40to72", 2, 3, 20, 36, 40, 72, options=WG, refused=True),
    Case("refused-dilated-24-couts-3x20x12x40to24", 1, 3, 20, 12, 40, 24, dilation=2, options=WG, refused=True),
    Case("refused-dilated-24-couts-3x20x12x40to24", 0, 3, 20, 12, 40, 24, dilation=2, options=WG, refused=True),
    Case("refused-dilated-20-couts-3x20x12x40to20", 1, 3, 20, 12, 40, 20, dilation=2, options=WG, refused=True),
    Case("refused-workspace-a-byte-short-3x20x36x40to72", 1, 3, 20, 36, 40, 72, tiled(FAST, 4, 9, 1, 2, 1, 4, 7, _ws(4, 72, 9, 40), red=1), options=WG,
         refused=True, ws_short=1),
    Case("refused-workspace-a-byte-short-3x20x12x40to72", 0, 3, 20, 12, 40, 72, tiled(GENERIC, 4, 9, 1, 1, 1, 3, 6, _ws(3, 72, 9, 40), red=1), options=WG,
         refused=True, ws_short=1),
]


# ---- the launch of a case (host logic: the queries run without a GPU) ----------------------------------------------------------------
def descriptor(L, case):
    return conv_desc(L, case.code, case.n, case.h, case.w, case.c0, case.cout, case.k, case.stride, case.pad, c1=case.c1, up0=case.up0,
                     groups=case.c0 // case.cg if case.cg else 0, dilation=case.dilation if case.dilation > 1 else 0)


def plan_of(pl):
    """the library's vs_wgrad_plan as a Plan"""
    return Plan(*(int(getattr(pl, f)) for f in PLAN_FIELDS))


def queried(L, case):
    """(status, Plan) the library answers for the case under the case's options"""
    with option(**dict(case.options)):
        pl = L.WgradPlan()
        if case.classes:
            rc = L.lib.vs_head_wgrad_planes_variant(case.code, case.n, case.classes, case.h, case.w, pl)
        else:
            rc = L.lib.vs_conv2d_wgrad_variant(descriptor(L, case), pl)
        return rc, plan_of(pl)


def queried_plan(L, d):
    """the plan the library answers for a descriptor under the current options - for the tests that have no table row"""
    pl = L.WgradPlan()
    assert L.lib.vs_conv2d_wgrad_variant(d, pl) == 0, L.last_error()
    return plan_of(pl)


def launch_figure(L, d, got, x0, x1, dy, plan=None):
    """max |got - ref| / bound for a launch of descriptor d that wrote `got`, on the NCHW operands x0, x1, dy the storage type holds exactly;
    plan: what queried_plan answered when the launch ran (default: what it answers now)"""
    ref, bound = reference_and_bound(d.dtype, x0, x1, dy, plan or queried_plan(L, d), k=d.kh, up0=d.up0, stride=d.stride, pad=d.pad,
                                     dilation=max(d.dilation, 1), groups=max(d.groups, 1))
    return figure_against(got.detach().cpu().reshape(ref.shape), ref, bound)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def inputs(case):
    """x0 (the stored source: half resolution when up0 = 1), x1 or None, dy (n, cout, hout, wout; the planes form: n, classes, h, w) - fp32
    CPU tensors in NCHW, N(0, 1), whose values the case's storage type holds exactly (the gradient planes: bf16, what the kernel rounds
    them to)"""
    g = torch.Generator().manual_seed(case.seed)
    code = 1 if case.code == 2 else case.code
    sh = 1 if case.up0 == 1 else 0
    x0 = rounded(torch.randn(case.n, case.c0, case.h >> sh, case.w >> sh, generator=g), code)
    x1 = rounded(torch.randn(case.n, case.c1, case.h, case.w, generator=g), code) if case.c1 else None
    dy = rounded(torch.randn(case.n, case.classes or case.cout, case.hout, case.wout, generator=g), code)
    return x0, x1, dy


# ---- the reference and the bound ---------------------------------------------------------------------------------------------------
def _wgrad(src, dy, k, stride, pad, dilation, groups):
    """d sum(conv2d(src, w) * dy) / dw for the k x k kernel w, over the dilated kernel written out with its zeros; (cout, cin / groups, k, k)"""
    wd = dilated(torch.zeros(dy.shape[1], src.shape[1] // groups, k, k, dtype=src.dtype), dilation).requires_grad_()
    (F.conv2d(src, wd, stride=stride, padding=pad, groups=groups) * dy).sum().backward()
    return wd.grad[:, :, ::dilation, ::dilation].contiguous()


def chain_roundings(code, plan):
    """m of the module docstring for a launch of dtype `code` that runs `plan` (reduce_group: the reduce the launch takes)"""
    kstep, per = KSTEP[code], plan.tiles_per_split
    if plan.family == ROWS:
        steps, combine = per * plan.wq * (2 if plan.rows_form == 2 else 1), 3
    elif plan.family == RING:
        steps, combine = per * 4, 0
    elif plan.family == FAST:
        kg = 2 if plan.taps == 1 else 1
        steps, combine = per * -(-2 * plan.pt // kg), kg - 1
    else:
        wk = 4 // plan.wo
        steps, combine = per * -(-(64 * plan.pt // kstep) // wk), wk - 1
    m = 4 * steps if code == 0 else kstep + steps - 1
    return m + combine + reduce_depth(plan.reduce_group, plan.nsplit)


def reduce_depth(group, nsplit):
    """roundings a slab can meet in the slab reduce"""
    if group < 0 or nsplit <= 1:
        return 0
    lanes, tree = (4, 2) if group == 0 else (group, group - 1)
    slabs = -(-nsplit // lanes)
    return min(-(-slabs // 2) + 1 + tree, nsplit - 1)


def reference_and_bound(code, x0, x1, dy, plan, *, k=3, up0=0, stride=1, pad=0, dilation=1, groups=1, reduce_group=None):
    """(reference, bound) in float64, laid out as the launch writes dw: [cout][taps][cin / groups].  x0, x1, dy: NCHW tensors whose values
    the storage type holds exactly.  plan: the Plan of the launch (a table row's hand-written one; a test without a table takes the
    query's); reduce_group overrides the plan's where the launch's buffers are off alignment."""
    if reduce_group is not None and reduce_group != plan.reduce_group:
        plan = dataclasses.replace(plan, reduce_group=reduce_group)
    src, d64 = source(x0, x1, up0).double(), dy.double()
    ref = _wgrad(src, d64, k, stride, pad, dilation, groups)
    mag = _wgrad(src.abs(), d64.abs(), k, stride, pad, dilation, groups)
    err = gamma(chain_roundings(code, plan)) * mag
    bound = err + (U * (ref.abs() + err)).clamp_min(2.0 ** -150)
    return _layout(ref), _layout(bound)


def _layout(t):
    return t.permute(0, 2, 3, 1).reshape(t.shape[0], t.shape[2] * t.shape[3], t.shape[1]).contiguous()


def _groups(case):
    return case.c0 // case.cg if case.cg else 1


@functools.lru_cache(maxsize=4)
def reference(case):
    """(reference, bound) of the case in the layout of case.dw_shape"""
    x0, x1, dy = inputs(case)
    return reference_and_bound(case.code, x0, x1, dy, case.plan, k=case.k, up0=case.up0, stride=case.stride, pad=case.pad, dilation=case.dilation,
                               groups=_groups(case), reduce_group=case.reduce_group)


def figure_against(got, ref, bound):
    return worst((got.double() - ref).abs(), bound)


def figure(got, case):
    """max over the elements of |got - ref| / bound; got on the CPU in the layout the launch writes"""
    ref, bound = reference(case)
    assert tuple(got.shape) == tuple(ref.shape), (got.shape, ref.shape)
    return figure_against(got, ref, bound)


def old_tolerance(case):
    """per element what the assertions before this table allowed: rtol 1e-3, atol 1e-3 * max |ref|"""
    ref, _ = reference(case)
    return 1e-3 * ref.abs().max() + 1e-3 * ref.abs()


def independent_reference(case):
    """the float64 weight gradient once more, by another route: F.unfold (with its own dilation and stride) over the explicitly built
    source, one image at a time, and an einsum with the gradient over the pixels; a grouped layer one group at a time"""
    x0, x1, dy = inputs(case)
    src, d64 = source(x0, x1, case.up0).double(), dy.double()
    groups, cout = _groups(case), dy.shape[1]
    cg_in, cg_out = src.shape[1] // groups, cout // groups
    out = torch.zeros(cout, cg_in * case.k * case.k, dtype=torch.float64)
    for i in range(case.n):
        for g in range(groups):
            cols = F.unfold(src[i:i + 1, g * cg_in:(g + 1) * cg_in], case.k, dilation=case.dilation, padding=case.pad, stride=case.stride)[0]
            out[g * cg_out:(g + 1) * cg_out] += torch.einsum("ol,kl->ok", d64[i, g * cg_out:(g + 1) * cg_out].reshape(cg_out, -1), cols)
    return _layout(out.view(cout, cg_in, case.k, case.k))


# ---- fp32 on the CPU: an honest evaluation and the mutations the bound must catch -------------------------------------------------
def split_pixels(case):
    """the plan's K splits as lists of pixel tiles, each tile a (image slice, row slice, column slice) of dy - the tile order and the
    tile shapes of geom(); a row kernel's tile is one row step (one gradient row; behind the upsampling: the two of a source row)"""
    p = case.plan
    if p.family == ROWS:
        rows = 2 if p.rows_form == 2 else 1
        steps = case.n * case.hout // rows
        tiles = [(slice(s * rows // case.hout, s * rows // case.hout + 1), slice(s * rows % case.hout, s * rows % case.hout + rows), slice(None))
                 for s in range(steps)]
    elif p.imgs == 2:
        tiles = [(slice(2 * t, 2 * t + 2), slice(None), slice(None)) for t in range(case.n // 2)]
    else:
        tw = (16 if p.pt == 2 else 8) if case.stride == 1 else (16 if case.wout >= 16 else 8)
        th = 64 * p.pt // tw
        tiles = [(slice(i, i + 1), slice(ty * th, (ty + 1) * th), slice(tx * tw, (tx + 1) * tw))
                 for i in range(case.n) for ty in range(-(-case.hout // th)) for tx in range(-(-case.wout // tw))]
    per = p.tiles_per_split
    return [tiles[s:s + per] for s in range(0, len(tiles), per)]


def _masked(dy, tiles):
    out = torch.zeros_like(dy)
    for t in tiles:
        out[t[0], :, t[1], t[2]] = dy[t[0], :, t[1], t[2]]
    return out


def cpu_fp32(case, mutation=None):
    """fp32 autograd on the CPU, laid out as the launch writes.  mutation:
    "tail"   one pixel's last 8 input channels (4 for fp32) are dropped at one tap - the last gradient pixel (last image, last row,
             last column) at the centre tap;
    "tile"   the last tile of the first split is dropped;
    "slab"   the last split's slab is left out of the sum (launches with more than one split)."""
    x0, x1, dy = inputs(case)
    src = source(x0, x1, case.up0)
    args = (case.k, case.stride, case.pad, case.dilation, _groups(case))
    dw = _wgrad(src, dy, *args)
    if mutation == "tail":
        drop = 4 if case.code == 0 else 8
        one = torch.zeros_like(dy)
        one[-1, :, -1, -1] = dy[-1, :, -1, -1]
        part = _wgrad(src, one, *args)
        c = case.k // 2
        dw[:, -drop:, c, c] -= part[:, -drop:, c, c]
    elif mutation in ("tile", "slab"):
        splits = split_pixels(case)
        assert len(splits) == case.plan.nsplit, (len(splits), case.plan.nsplit)
        gone = splits[0][-1:] if mutation == "tile" else splits[-1]
        dw = dw - _wgrad(src, _masked(dy, gone), *args)
    elif mutation is not None:
        raise ValueError(mutation)
    return _layout(dw)
