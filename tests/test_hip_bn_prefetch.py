"""-m gpu: the `bn_prefetch` forms of the BatchNorm sweeps (csrc/norm.hip: the first trip's row and parameter loads issued before
the statistics prologue) against the forms without it.  Only the order in which loads are issued differs, so everything is
compared bit for bit between `bn_prefetch` 0 and 1 in one process; one shape per dtype is also held to the torch reference of
test_hip_ops.test_batchnorm_train_fwd_bwd at that test's tolerance, so that both arms being wrong together cannot pass.  The
stand-alone operators of the first test (two-sweep path, plain apply) pin that the option leaves their results alone.  The inline
sweeps, the ones that take the prefetch forms, are run as the network's plan reaches them (second test) and directly through the
seams vs_bn_apply_from_partials, vs_bn_apply_from_bins and vs_bn_bwd_from_partials (third test), where one case per seam is also
held to the float64 figures of tests/batchnorm_cases.py."""
import functools

import pytest
import torch
import torch.nn.functional as F

import batchnorm_cases as B
from hip_helpers import DEV, lib, rounded, sync, tdtype, tol
from hip_helpers import option as _option

pytestmark = pytest.mark.gpu
CODES = [0, 1]
# (rows, c): rows smaller than one trip and empty blocks; cv = 3, rpb = 85 (thread 255 is idle and must not prefetch); a plain
# multi-block case; rpb = 5 with 16 idle threads, several blocks and a ragged tail; rpb = 1
SHAPES = [(1, 8), (37, 24), (1000, 64), (4100, 384), (130, 2048)]
REF_SHAPE = (1000, 64)


@functools.lru_cache(maxsize=None)
def _case(rows, c, code):
    """inputs of one operator case on the CPU (fp32 values the device dtype holds exactly), built once"""
    g = torch.Generator().manual_seed(1000 * c + rows + code)
    x = rounded(torch.randn(rows, c, generator=g) * 2 + 0.5, code)
    res = rounded(torch.randn(rows, c, generator=g), code)
    dy = rounded(torch.randn(rows, c, generator=g), code)
    gamma, beta = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g)
    return x, res, dy, gamma, beta


@functools.lru_cache(maxsize=None)
def _torch_reference(code):
    """y = relu(bn(x) + res) and its gradients, as test_batchnorm_train_fwd_bwd forms them ([rows][c] viewed as N = 1, H = rows, W = 1)"""
    rows, c = REF_SHAPE
    x, res, dy, gamma, beta = _case(rows, c, code)
    nchw = lambda t: t.t().reshape(1, c, rows, 1)
    xr, rr = nchw(x).clone().requires_grad_(), nchw(res).clone().requires_grad_()
    gr, br = gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    y = (F.batch_norm(xr, None, None, gr, br, training=True, momentum=0.1, eps=1e-5) + rr).relu()
    y.backward(nchw(dy))
    back = lambda t: t.reshape(c, rows).t()
    return back(xr.grad), back(rr.grad), gr.grad, br.grad


def _bwd(L, code, variant, with_dres, dev, fill):
    """one vs_bn_bwd / vs_bn_bwd_recompute call; outputs start from `fill` so that an element no thread wrote shows"""
    xd, yd, dyd, mean, invstd, gd, bd, ws, wsb, rows, c = dev
    dx = torch.full_like(xd, fill)
    dres = torch.full_like(xd, fill) if with_dres else None
    dgamma, dbeta = torch.full((c,), fill, device=DEV), torch.full((c,), fill, device=DEV)
    if variant == "recompute":      # mask recomputed from x and beta (units without a residual input)
        L.check(L.lib.vs_bn_bwd_recompute(code, L.ptr(dyd), None, L.ptr(xd), L.ptr(mean), L.ptr(invstd), L.ptr(gd), L.ptr(bd), 1,
                                          L.ptr(dx), L.ptr(dres), L.ptr(dgamma), L.ptr(dbeta), rows, c, L.ptr(ws), wsb, None))
    else:
        relu = 1 if variant == "relu_y" else 0
        L.check(L.lib.vs_bn_bwd(code, L.ptr(dyd), L.ptr(yd) if relu else None, L.ptr(xd), L.ptr(mean), L.ptr(invstd), L.ptr(gd), relu,
                                L.ptr(dx), L.ptr(dres), L.ptr(dgamma), L.ptr(dbeta), rows, c, L.ptr(ws), wsb, None))
    sync()
    return dx, dres, dgamma, dbeta


@pytest.mark.parametrize("code", CODES)
@pytest.mark.parametrize("rows,c", SHAPES)
def test_bn_backward_sweeps_same_bits_with_and_without_prefetch(rows, c, code):
    L = lib()
    x, res, dy, gamma, beta = _case(rows, c, code)
    dt = tdtype(code)
    xd, resd, dyd = x.to(DEV, dt), res.to(DEV, dt), dy.to(DEV, dt)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    wsb = L.lib.vs_bn_workspace(rows, c)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    mean, invstd = torch.empty(c, device=DEV), torch.empty(c, device=DEV)
    L.check(L.lib.vs_bn_stats(code, L.ptr(xd), rows, c, 1e-5, 0.1, L.ptr(mean), L.ptr(invstd), None, None, L.ptr(ws), wsb, None))
    yd = torch.empty_like(xd)
    L.check(L.lib.vs_bn_apply(code, L.ptr(xd), L.ptr(mean), L.ptr(invstd), L.ptr(gd), L.ptr(bd), L.ptr(resd), 1, L.ptr(yd), rows, c, None))
    sync()
    dev = (xd, yd, dyd, mean, invstd, gd, bd, ws, wsb, rows, c)
    for variant in ("plain", "relu_y", "recompute"):
        for with_dres in (False, True):
            with _option(bn_prefetch=0):
                old = _bwd(L, code, variant, with_dres, dev, 1.0)
            with _option(bn_prefetch=1):
                new = _bwd(L, code, variant, with_dres, dev, 2.0)
            for name, a, b in zip(("dx", "dres", "dgamma", "dbeta"), old, new):
                if a is None:
                    continue
                assert torch.equal(a, b), (variant, with_dres, name, (a.float() - b.float()).abs().max().item())
            if (rows, c) == REF_SHAPE and variant == "relu_y" and with_dres:
                rdx, rdres, rdgamma, rdbeta = _torch_reference(code)
                dx, dres, dgamma, dbeta = new
                assert torch.allclose(dres.float().cpu(), rdres, **tol(code, rdres.abs().max().item()))
                assert torch.allclose(dbeta.cpu(), rdbeta, rtol=1e-3, atol=1e-3 * rdbeta.abs().max().item())
                assert torch.allclose(dgamma.cpu(), rdgamma, rtol=2e-3, atol=2e-3 * rdgamma.abs().max().item() + (0 if code == 0 else 0.05))
                assert torch.allclose(dx.float().cpu(), rdx, **tol(code, rdx.abs().max().item()))


def _two_steps(precision):
    """two eager training steps (fused AdamW) of U-Net / ResNet-34, 2 classes, batch 3, 96 x 64: the odd batch and layer4's 3 x 2 map
    give ragged trips and c up to 512 (both bin-sum paths of the inline forward)"""
    from volume_segmantics_amd.data.losses import HipDiceLoss
    from volume_segmantics_amd.engine import VolSegUnet
    g = torch.Generator().manual_seed(21)
    x = torch.randn(3, 1, 96, 64, generator=g).to(DEV)
    t = torch.nn.functional.one_hot((torch.rand(3, 96, 64, generator=g) > 0.6).long(), 2).permute(0, 3, 1, 2).float().contiguous().to(DEV)
    model = VolSegUnet(2, device=DEV, precision=precision, seed=7)
    opt = model.fused_adamw(lr=1e-3, fuse_step_into_backward=True)
    model.train()
    crit = HipDiceLoss()
    losses = []
    for _ in range(2):
        opt.zero_grad()
        loss = crit(model(x), t)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    sync()
    return losses, model._flat.clone(), model._flat_grad.clone(), model._bnstate.clone()


# the inline forms as the network's plan reaches them: the default plan (fixed-point bins), fp32 partial rows inline
# (stats_bins 0) and finalize + plain apply everywhere (bn_inline_rows 0)
@pytest.mark.parametrize("precision,pinned", [("bf16", {}), ("fp32", {}), ("bf16", {"stats_bins": 0}), ("bf16", {"bn_inline_rows": 0})])
def test_training_steps_same_bits_with_and_without_prefetch(precision, pinned):
    with _option(**pinned):
        with _option(bn_prefetch=0):
            old = _two_steps(precision)
        with _option(bn_prefetch=1):
            new = _two_steps(precision)
    assert old[0] == new[0], (old[0], new[0])
    assert all(l == l for l in new[0]) and torch.isfinite(new[1]).all()
    for name, a, b in zip(("_flat", "_flat_grad", "_bnstate"), old[1:], new[1:]):
        assert torch.equal(a, b), (precision, pinned, name, (a - b).abs().max().item())


# ---- the inline sweeps through their seams ------------------------------------------------------------------------------------------
# Each shape is the smallest at which another branch or a ragged edge is taken.  Forward from partial rows: the shapes of the first
# test; c = 24 and 384 fail 256 % (2 c / 4) == 0 and c = 2048 exceeds 512 (the per-channel sum), the others take the all-threads sum.
# Forward from bins: 2 c <= 256 sums by row groups, c = 512 by columns.  Backward: up to 64 rows are summed inside the apply sweep, 65
# rows take bn_bwd_finalize and the plain apply sweep, which the option must leave alone.
NSTATS = (1, 3, 64)
BINS_SHAPES = [(37, 8), (1000, 64), (300, 512)]
BWD_SHAPES = [(1, 8), (37, 8), (1000, 64), (4100, 512)]
BWD_NPARTS = NSTATS + (65,)
REF_NSTATS = 3


def _held(figures, context):
    """figures of batchnorm_cases.py: measured error over bound (or a distance in ulps), at most 1"""
    failed = [(label, ratio) for label, ratio in figures if not ratio <= 1.0]
    assert not failed, (context, failed)


def _both_arms(run, names, context):
    """run(fill) under bn_prefetch 0 and 1, outputs prefilled with two different constants; equal bits, and the second arm's outputs"""
    with _option(bn_prefetch=0):
        old = run(1.0)
    with _option(bn_prefetch=1):
        new = run(2.0)
    for name, a, b in zip(names, old, new):
        if a is not None:
            assert torch.equal(a, b), (context, name, (a.float() - b.float()).abs().max().item())
    return new


def _inline_forward(L, source, code, rows, c, nstats, full, held):
    """one forward seam on one case, both arms; full = residual + ReLU; held: also against float64"""
    x, res, gamma, beta, rm0, rv0 = (t.to(DEV) for t in B.inline_inputs(c, rows, code)[:6])
    s, q = x.double().sum(0).cpu(), (x.double() ** 2).sum(0).cpu()
    if source == "bins":
        stats, tot = B.split_bins(s, q, nstats, nstats + c)
        s_tot, q_tot = tot[0].double() / L.lib.vs_stat_scale(0), tot[1].double() / L.lib.vs_stat_scale(1)
    else:
        stats = B.split_rows(s, q, nstats, nstats + c)
        s_tot, q_tot = stats[:, 0].double().sum(0), stats[:, 1].double().sum(0)
    stats = stats.to(DEV)
    dt = tdtype(code)
    xd, resd = x.to(dt), res.to(dt)

    def run(fill):
        y, mean, invstd = torch.full_like(xd, fill), torch.full((c,), fill, device=DEV), torch.full((c,), fill, device=DEV)
        rm, rv = rm0.clone(), rv0.clone()
        r, relu = (L.ptr(resd), 1) if full else (None, 0)
        if source == "bins":
            L.check(L.lib.vs_bn_apply_from_bins(code, L.ptr(xd), L.ptr(stats), nstats, 1e-5, 0.1, L.ptr(mean), L.ptr(invstd), L.ptr(rm), L.ptr(rv),
                                                L.ptr(gamma), L.ptr(beta), r, relu, L.ptr(y), rows, c, 0, None))
        else:
            L.check(L.lib.vs_bn_apply_from_partials(code, L.ptr(xd), L.ptr(stats), nstats, 1e-5, 0.1, L.ptr(mean), L.ptr(invstd), L.ptr(rm), L.ptr(rv),
                                                    L.ptr(gamma), L.ptr(beta), r, relu, L.ptr(y), rows, c, None))
        sync()
        return y, mean, invstd, rm, rv

    context = (source, rows, c, nstats, full, code)
    y, mean, invstd, rm, rv = _both_arms(run, ("y", "mean", "invstd", "running_mean", "running_var"), context)
    if held:
        want = B.defined_stats(s_tot.to(DEV), q_tot.to(DEV), rows, 1e-5, 0.1, rm0, rv0)
        _held(B.published_figures(source, want, (mean, invstd, rm, rv)) +
              B.apply_figures(f"{source} y", x, res if full else None, int(full), gamma, beta, mean, invstd, y, code), context)


def _inline_backward(L, code, rows, c, nparts, with_dres, held):
    """vs_bn_bwd_from_partials on one case, both arms; held: also against float64"""
    x, _, gamma, _, _, _, g, mean, invstd = (t.to(DEV) for t in B.inline_inputs(c, rows, code))
    g64 = g.double()
    xhat = (x.double() - mean.double()) * invstd.double()
    stats = B.split_rows(g64.sum(0).cpu(), (g64 * xhat).sum(0).cpu(), nparts, nparts + c).to(DEV)
    dt = tdtype(code)
    xd, gd = x.to(dt), g.to(dt)

    def run(fill):
        dx = torch.full_like(xd, fill)
        dres = torch.full_like(xd, fill) if with_dres else None
        dgamma, dbeta = torch.full((c,), fill, device=DEV), torch.full((c,), fill, device=DEV)
        L.check(L.lib.vs_bn_bwd_from_partials(code, L.ptr(gd), L.ptr(xd), L.ptr(mean), L.ptr(invstd), L.ptr(gamma), L.ptr(dx), L.ptr(dres),
                                              L.ptr(dgamma), L.ptr(dbeta), rows, c, L.ptr(stats), nparts, None))
        sync()
        return dx, dres, dgamma, dbeta

    context = ("bwd", rows, c, nparts, with_dres, code)
    dx, dres, dgamma, dbeta = _both_arms(run, ("dx", "dres", "dgamma", "dbeta"), context)
    if held:
        want_db, want_dg = stats[:, 0].double().sum(0).float(), stats[:, 1].double().sum(0).float()
        _held([("bwd dbeta ulps", float(B.ulps(dbeta, want_db))), ("bwd dgamma ulps", float(B.ulps(dgamma, want_dg)))] +
              B.dx_figures("bwd", g64, x, mean, invstd, gamma, dgamma, dbeta, dx, dres, code), context)


@pytest.mark.parametrize("code", CODES, ids=["fp32", "bf16"])
def test_inline_sweeps_same_bits_with_and_without_prefetch(code):
    """the three seams of the inline sweeps driven directly, every output bit for bit between bn_prefetch 0 and 1; the case (1000, 64)
    in bf16 of each seam is also held to its float64 figures at the bounds of batchnorm_cases.py (two arms wrong together must not pass)"""
    L = lib()
    for source, shapes in (("partials", SHAPES), ("bins", BINS_SHAPES)):
        for rows, c in shapes:
            for nstats in NSTATS:
                for full in (False, True):
                    _inline_forward(L, source, code, rows, c, nstats, full, held=(rows, c) == REF_SHAPE and code == 1 and nstats == REF_NSTATS and full)
    for rows, c in BWD_SHAPES:
        for nparts in BWD_NPARTS:
            for with_dres in (False, True):
                _inline_backward(L, code, rows, c, nparts, with_dres, held=(rows, c) == REF_SHAPE and code == 1 and nparts == REF_NSTATS and with_dres)
