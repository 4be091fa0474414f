"""-m gpu: the `bn_prefetch` forms of the BatchNorm sweeps (csrc/norm.hip: the first trip's row and parameter loads issued before
the statistics prologue) against the forms without it.  Only the order in which loads are issued differs, so everything is
compared bit for bit between `bn_prefetch` 0 and 1 in one process; one shape per dtype is also held to the torch reference of
test_hip_ops.test_batchnorm_train_fwd_bwd at that test's tolerance, so that both arms being wrong together cannot pass.  The
inline sweeps, the ones that take the prefetch forms, are reachable only from the network's plan (second test); the stand-alone
operators of the first test (two-sweep path, plain apply) pin that the option leaves their results alone."""
import functools

import pytest
import torch
import torch.nn.functional as F

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


# the inline forms are reachable only from the network's plan: the default plan (fixed-point bins), fp32 partial rows inline
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
