"""-m gpu: every instantiation the weight-gradient launch of csrc/conv_wgrad.hip can select (tests/wgrad_cases.py: the generic, fast, ring
and row-streaming kernels, the slab-reduce kernels and the grouped extract, with their loader forms and split structures), one small
launch each through the C ABI, against the float64 CPU reference of the same operands: the plan query answers the table's structure,
the launch writes every element of dw (prefilled with NaN) and nothing in the guard bands around dw and around a workspace of exactly
the queried size, the error stays within the per-element bound derived in wgrad_cases.py - for fp32 within hip_helpers.tol as well -
and a second launch gives the same bits.  The launches the table says must be refused return an error and write nothing."""
import pytest
import torch

import wgrad_cases as WC
from hip_helpers import DEV, lib, option, sync, to_nhwc, tol

pytestmark = pytest.mark.gpu
SENTINEL = -77.0
BAND = 256                # floats on either side: a multiple of 64, so the interior keeps the allocation's alignment


class Guarded:
    """`count` floats of NaN inside a larger fp32 buffer, SENTINEL in a band before and after them; shift: floats the interior is moved
    off the buffer's 16-byte alignment"""
    def __init__(self, count, shift=0):
        self.buf = torch.full((count + 2 * BAND + shift,), SENTINEL, device=DEV, dtype=torch.float32)
        self.lo, self.hi = BAND + shift, BAND + shift + count
        self.out = self.buf[self.lo:self.hi]
        self.out.fill_(float("nan"))

    def bands_untouched(self):
        edge = torch.cat([self.buf[:self.lo], self.buf[self.hi:]])
        return bool(torch.equal(edge.view(torch.int32), torch.full_like(edge, SENTINEL).view(torch.int32)))

    def bits(self):
        return self.buf.view(torch.int32).clone()


def _operands(case):
    x0, x1, dy = WC.inputs(case)
    x0d, x1d = to_nhwc(x0, case.code), (to_nhwc(x1, case.code) if x1 is not None else None)
    dyd = dy.contiguous().to(DEV) if case.classes else to_nhwc(dy, case.code)          # the head's planes: fp32 NCHW as autograd hands them over
    return x0d, x1d, dyd


def _launch(L, case, ops, dw, ws, ws_bytes):
    x0d, x1d, dyd = ops
    if case.classes:
        rc = L.lib.vs_head_wgrad_planes(case.code, L.ptr(x0d), L.ptr(dyd), L.ptr(dw.out), L.ptr(ws.out), ws_bytes, case.n, case.classes, case.h, case.w, None)
    else:
        rc = L.lib.vs_conv2d_wgrad(WC.descriptor(L, case), L.ptr(x0d), L.ptr(x1d), L.ptr(dyd), L.ptr(dw.out), L.ptr(ws.out), ws_bytes, None)
    sync()
    return rc


def _count(shape):
    n = 1
    for s in shape:
        n *= s
    return n


@pytest.mark.parametrize("case", WC.CASES, ids=lambda c: c.id)
def test_weight_gradient_within_the_per_element_bound(case):
    L = lib()
    ops = _operands(case)
    assert case.plan.workspace_bytes % 4 == 0
    runs = []
    with option(**dict(case.options)):
        rc, plan = WC.queried(L, case)
        assert rc == 0 and plan == case.plan, (rc, plan)
        for _ in range(2):
            dw, ws = Guarded(_count(case.dw_shape)), Guarded(case.plan.workspace_bytes // 4, case.ws_shift)
            L.check(_launch(L, case, ops, dw, ws, case.plan.workspace_bytes))
            assert dw.bands_untouched(), "the launch wrote outside dw"
            assert ws.bands_untouched(), "the launch wrote outside the workspace it asked for"
            runs.append(dw.out.clone())
    got = runs[0].cpu().view(case.dw_shape)
    assert torch.isfinite(got).all(), f"{int((~torch.isfinite(got)).sum())} elements not written"
    fig = WC.figure(got, case)
    print(f"{case.id} [{case.family}]: {fig:.3g} of the bound")
    assert fig <= 1.0, (case.id, fig)
    if case.code == 0:
        ref, _ = WC.reference(case)
        assert torch.allclose(got, ref.float(), **tol(0, ref.abs().max().item())), (got - ref.float()).abs().max()
    assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32)), "two launches of the same operands differ"


@pytest.mark.parametrize("case", WC.REFUSED, ids=lambda c: c.id)
def test_refused_launch_returns_an_error_and_writes_nothing(case):
    L = lib()
    ops = _operands(case)
    with option(**dict(case.options)):
        rc, plan = WC.queried(L, case)
        assert (rc == 0 and plan == case.plan) if case.ws_short else rc != 0
        asked = case.plan.workspace_bytes if case.plan else max(L.lib.vs_conv2d_wgrad_workspace(WC.descriptor(L, case)), 1 << 20)
        dw, ws = Guarded(_count(case.dw_shape)), Guarded(asked // 4)
        before = dw.bits(), ws.bits()
        rc = _launch(L, case, ops, dw, ws, asked - case.ws_short)
    assert rc != 0 and L.last_error()
    assert torch.equal(dw.bits(), before[0]) and torch.equal(ws.bits(), before[1])
