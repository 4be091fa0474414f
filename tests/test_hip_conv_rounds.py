"""-m gpu: what hoisting the epilogue's loads in front of its stores can break (csrc/conv_common.h conv_epilogue, csrc/conv_ring.h,
csrc/conv_wgrad_ring.h).  Since every global load of an epilogue is issued before its first store, a load also runs on lanes and cout
sub-tiles the stores skip - ragged tiles on both edges, a ragged cout tail - and a residual that IS the output is read before any of
it is written.  So: the smallest launches that select each kernel family (asserted through vs_conv2d_train_variant), in every
epilogue form, with z, y, residual, out and the partial rows each between NaN-filled guard bands, out NaN-prefilled, against a
float64 computation held to the per-element bound of tests/conv_cases.py, and every launch repeated bit for bit.

The arithmetic and the dispatch have their own tests (test_hip_conv_bounds.py, test_hip_ring_kernels.py, test_conv_host.py); the shapes
here are the issue's, with the batch raised until the query reports the intended kernel: the ring kernel starts at 224 workgroups
(64-cout tiles) / 128 (32-cout tiles) (ring_mode, csrc/conv_igemm.hip).

Partial rows.  Row t holds, per channel, sum g and sum g * xhat over the tile's pixels, g = the STORED (rounded) gradient, xhat =
(z - mean) * invstd in fp32.  Against the float64 sums of the stored gradient the only error is fp32 summation and the fp32 evaluation
of a term: a term g * (z - mean) * invstd meets 3 roundings (z, mean, invstd are exact inputs), a sum of m terms in any order at most
m - 1 more per term.  m <= 256 pixels a tile, so per channel |sum - ref| <= gamma(256 + 3) * sum |term|, U = 2^-24; the rows are added
up in float64 here.  No absolute slack."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

import conv_cases as CC
import wgrad_cases as WC
from hip_helpers import DEV, conv_desc, lib, option, rounded, sync

pytestmark = pytest.mark.gpu
BF = 1
GUARD = 256            # elements of NaN on either side of a tensor (a multiple of every vector width)


@functools.lru_cache(maxsize=None)
def _shapes():
    # label: (n, h, w, cin, cout, options, plan code, partial rows)
    return {
        "ring32-16x20x20x128to40": (16, 20, 20, 128, 40, (), 32296, 64),            # ragged tiles on both edges, ragged cout tail
        "ring64-56x20x20x128to64": (56, 20, 20, 128, 64, (), 64296, 224),
        "pairs-4x8x8x128to64": (4, 8, 8, 128, 64, (), 32296, 2),                    # two 8 x 8 images a tile
        "tile64-1x20x20x64to64": (1, 20, 20, 64, 64, CC.SMALL, 64298, 4),           # the 64-cout tile kernel: four cout sub-tiles
    }


SHAPES = list(_shapes())
# (fused BatchNorm-backward epilogue?, ReLU mask: None / "y" (from the activation) / "z" (recomputed from z), residual: None / "separate" / "in-place")
MODES = ([pytest.param((False, None, r), id="plain" + s) for r, s in ((None, ""), ("separate", "+residual"), ("in-place", "+residual-in-place"))] +
         [pytest.param((True, m, r), id=f"bnbwd-{ms}-{rs}")
          for m, ms in ((None, "nomask"), ("y", "mask-from-y"), ("z", "mask-recomputed"))
          for r, rs in ((None, "sole"), ("separate", "residual"), ("in-place", "residual-in-place"))])


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


class Guarded:
    """a device tensor between two NaN-filled guard bands"""
    def __init__(self, values, dtype):
        flat = values.reshape(-1).to(dtype)
        self.buf = torch.full((flat.numel() + 2 * GUARD,), float("nan"), dtype=dtype, device=DEV)
        self.view = self.buf[GUARD:GUARD + flat.numel()]
        self.view.copy_(flat)
        self.shape = values.shape

    def ptr(self):
        return self.view.data_ptr()

    def untouched(self):
        return bool(torch.isnan(self.buf[:GUARD]).all() and torch.isnan(self.buf[-GUARD:]).all())

    def bits(self):
        return self.buf.view(torch.int16 if self.buf.element_size() == 2 else torch.int32).clone()

    def values(self):
        return self.view.float().cpu().reshape(self.shape)


@functools.lru_cache(maxsize=2)
def _operands(label):
    """x, w, residual, z, y, mean, invstd, gamma, beta (fp32 CPU, NCHW; the 16-bit tensors hold bf16 values)"""
    n, h, w, cin, cout, *_ = _shapes()[label]
    g = torch.Generator().manual_seed(sum(map(ord, label)))
    x = rounded(torch.randn(n, cin, h, w, generator=g), BF)
    wt = rounded(torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5, BF)
    res = rounded(torch.randn(n, cout, h, w, generator=g), BF)
    z = rounded(torch.randn(n, cout, h, w, generator=g) * 1.5 + 0.2, BF)
    mean, invstd = z.mean((0, 2, 3)), 1 / torch.sqrt(z.var((0, 2, 3), unbiased=False) + 1e-5)
    gamma, beta = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.3
    bc = lambda v: v.view(1, -1, 1, 1)
    pre = (z - bc(mean)) * bc(invstd * gamma) + bc(beta)
    z = torch.where(pre.abs() < 1e-3, rounded(z + 0.5, BF), z)      # keep the recomputed pre-activation clear of zero: fp32 must not flip a mask bit
    pre = (z - bc(mean)) * bc(invstd * gamma) + bc(beta)
    assert not (pre.abs() < 1e-5).any()
    y = rounded(F.relu(pre + torch.randn(pre.shape, generator=g)), BF)      # a residual unit's activation: the mask is y > 0
    return x, wt, res, z, y, mean, invstd, gamma, beta, pre


@functools.lru_cache(maxsize=4)
def _reference(label, with_residual):
    """float64 value and per-element bound of conv (+ residual), stored as bf16 (tests/conv_cases.py)"""
    x, wt, res, *_ = _operands(label)
    return CC.reference_and_bound(BF, x, None, wt, pad=1, residual=res if with_residual else None)


def _launch(L, d, t, xd, wd, res_ptr, out):
    L.check(L.lib.vs_conv2d_train(d, xd.data_ptr(), None, wd.data_ptr(), res_ptr, out.ptr(), None, C.byref(t), None))
    sync()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("label", SHAPES)
def test_epilogue_loads_in_front_of_the_stores(label, mode):
    L = lib()
    n, h, w, cin, cout, options, code, rows = _shapes()[label]
    x, wt, res, z, y, mean, invstd, gamma, beta, pre = _operands(label)
    fused, mask, residual = mode
    in_place, with_res = residual == "in-place", residual is not None
    ref, bound = _reference(label, with_res)
    keep = torch.ones_like(ref, dtype=torch.bool) if mask is None else ((y > 0) if mask == "y" else (pre > 0))
    ref = ref * keep
    nan_out = torch.full((n, h, w, cout), float("nan"))
    with option(**dict(options)):
        d = conv_desc(L, BF, n, h, w, cin, cout, 3, 1, 1)
        t = L.ConvTrain()
        xd, wd = _nhwc(x).to(DEV, torch.bfloat16), _nhwc(wt).to(DEV, torch.bfloat16)
        zg, yg = Guarded(_nhwc(z), torch.bfloat16), Guarded(_nhwc(y), torch.bfloat16)
        vec = [v.to(DEV) for v in (mean, invstd, gamma, beta)]
        if fused:
            t.bz, t.bmean, t.binvstd = zg.ptr(), vec[0].data_ptr(), vec[1].data_ptr()
            t.brelu = 0 if mask is None else 1
            if mask == "y":
                t.by = yg.ptr()
            if mask == "z":
                t.bgamma, t.bbeta = vec[2].data_ptr(), vec[3].data_ptr()
            assert L.lib.vs_conv2d_stat_rows(d, t) == rows
        assert L.lib.vs_conv2d_train_variant(d, t) == code, (L.lib.vs_conv2d_train_variant(d, t), code)
        runs = []
        for _ in range(2):
            part = Guarded(torch.full((rows, 2, cout), float("nan")), torch.float32)
            if fused:
                t.bstats_partial = part.ptr()
            resg = Guarded(_nhwc(res), torch.bfloat16)
            out = resg if in_place else Guarded(nan_out, torch.bfloat16)       # in place: the output starts as the earlier contributions
            _launch(L, d, t, xd, wd, resg.ptr() if with_res else None, out)
            for name, gb in (("z", zg), ("y", yg), ("residual", resg), ("out", out), ("partial rows", part)):
                assert gb.untouched(), f"{name}: a guard band was written"
            runs.append((out.bits(), part.bits(), out.values().permute(0, 3, 1, 2), part.values()))
    got, rows_got = runs[0][2], runs[0][3]
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "a repeat of the launch differs"
    fig = CC.figure_against(got, ref, bound)
    print(f"{label} {mode}: {fig:.3g} of the bound")
    assert fig <= 1.0, fig
    assert (got[~keep] == 0).all(), "masked-off elements must be exactly zero"
    if fused:
        xhat = (z.double() - mean.double().view(1, -1, 1, 1)) * invstd.double().view(1, -1, 1, 1)
        g64 = got.double()
        sums = rows_got.double().sum(0)
        tol = CC.gamma(256 + 3)
        for k, (term, what) in enumerate(((g64, "sum g"), (g64 * xhat, "sum g xhat"))):
            err, lim = (sums[k] - term.sum((0, 2, 3))).abs(), tol * term.abs().sum((0, 2, 3))
            worst = (err / lim.clamp_min(1e-300)).max().item()
            print(f"{label} {mode} {what}: {worst:.3g} of the bound")
            assert worst <= 1.0, (what, worst)


def test_ring_weight_gradient_exact_workspace_and_guarded_dw():
    """conv_wgrad_ring_kernel (its prologue now takes its arguments in one batch): 2 x 16 x 16, 64 -> 64, against float64 with the bound of
    tests/wgrad_cases.py; the workspace is exactly what vs_conv2d_wgrad_workspace asks for, dw sits between guard bands, a repeat gives
    the same bits"""
    L = lib()
    n, h, w, c = 2, 16, 16, 64
    g = torch.Generator().manual_seed(71)
    x = rounded(torch.randn(n, c, h, w, generator=g), BF)
    dy = rounded(torch.randn(n, c, h, w, generator=g), BF)
    d = conv_desc(L, BF, n, h, w, c, c, 3, 1, 1)
    plan = WC.queried_plan(L, d)
    assert plan.family == WC.RING, WC.FAMILY[plan.family]
    xd, dyd = _nhwc(x).to(DEV, torch.bfloat16), _nhwc(dy).to(DEV, torch.bfloat16)
    ws_bytes = L.lib.vs_conv2d_wgrad_workspace(d)
    runs = []
    for _ in range(2):
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
        dw = Guarded(torch.full((c, 9, c), float("nan")), torch.float32)
        L.check(L.lib.vs_conv2d_wgrad(d, xd.data_ptr(), None, dyd.data_ptr(), dw.ptr(), ws.data_ptr(), ws_bytes, None))
        sync()
        assert dw.untouched(), "dw: a guard band was written"
        runs.append((dw.bits(), dw.values()))
    fig = WC.launch_figure(L, d, runs[0][1], x, None, dy, plan)
    print(f"ring weight gradient: {fig:.3g} of the bound")
    assert fig <= 1.0, fig
    assert torch.equal(runs[0][0], runs[1][0])
