"""-m gpu: every instantiation the forward launch of csrc/conv_igemm.hip can select (tests/conv_cases.py: the tile family, the ring
kernel's three modes, the persistent stream kernel, the direct strip kernel and the head kernel, with their loader and epilogue
forms), one small launch each through the C ABI, against the float64 CPU reference of the same operands: the plan query answers the
table's code, the launch writes every output element (prefilled with NaN) and nothing in the guard bands around the output, and the
error stays within the per-element bound derived in conv_cases.py - for fp32 within hip_helpers.tol as well."""
import ctypes as C

import pytest
import torch

import conv_cases as CC
from hip_helpers import DEV, from_nhwc, lib, option, sync, tdtype, to_nhwc, tol, w_krsc

pytestmark = pytest.mark.gpu
SENTINEL = -77.0          # exact in every stored type


class Guarded:
    """an output tensor inside a larger buffer: NaN where the launch must write, SENTINEL in a band of at least one image row (rounded
    up to 64 elements: the vector stores stay aligned) before and after it"""
    def __init__(self, shape, dtype, row):
        self.band = -(-row // 64) * 64
        count = 1
        for s in shape:
            count *= s
        self.buf = torch.full((count + 2 * self.band,), SENTINEL, device=DEV, dtype=dtype)
        self.out = self.buf[self.band:self.band + count].view(shape)
        self.out.fill_(float("nan"))
        self.bits = torch.int32 if dtype == torch.float32 else torch.int16

    def bands_untouched(self):
        want = torch.full((self.band,), SENTINEL, device=DEV, dtype=self.buf.dtype).view(self.bits)
        return bool(torch.equal(self.buf[:self.band].view(self.bits), want) and torch.equal(self.buf[-self.band:].view(self.bits), want))


def _outputs(case):
    """the output buffers of the case, NHWC in the stored type (the head: fp32 NCHW)"""
    dt = tdtype(case.store_code)
    ho, wo = (case.hout // 2, case.wout // 2) if case.pool0 else (case.hout, case.wout)
    if case.out_f32 == 3:
        return [Guarded((case.n, case.cout, ho, wo), dt, wo)]
    if case.split_c:
        return [Guarded((case.n, ho, wo, c), dt, wo * c) for c in (case.split_c, case.cout - case.split_c)]
    return [Guarded((case.n, ho, wo, case.cout), dt, wo * case.cout)]


def _launch(L, case, outs):
    x0, x1, w, scale, shift, res = CC.inputs(case)
    keep = [to_nhwc(x0, case.code), to_nhwc(x1, case.code) if x1 is not None else None, w_krsc(w, case.code),
            scale.to(DEV) if scale is not None else None, shift.to(DEV) if shift is not None else None,
            to_nhwc(res, case.code) if res is not None else None]
    x0d, x1d, wd, sc, sh, rd = keep
    d = CC.descriptor(L, case)
    y, y1 = outs[0].out, (outs[1].out if len(outs) > 1 else None)
    if case.pool0:
        t = CC.train_block(L, case)
        rc = L.lib.vs_conv2d_train(d, L.ptr(x0d), L.ptr(x1d), L.ptr(wd), L.ptr(rd), L.ptr(y), L.ptr(y1), C.byref(t), None)
    else:
        rc = L.lib.vs_conv2d_fwd(d, L.ptr(x0d), L.ptr(x1d), L.ptr(wd), L.ptr(sc), L.ptr(sh), L.ptr(rd), L.ptr(y), L.ptr(y1), None)
    sync()
    return rc


@pytest.mark.parametrize("case", CC.CASES, ids=lambda c: c.id)
def test_conv_forward_within_the_per_element_bound(case):
    L = lib()
    outs = _outputs(case)
    with option(**dict(case.options)):
        code, rows = CC.queried(L, case)
        assert code == case.plan and (not case.stat_rows or rows == case.stat_rows), (code, rows)
        L.check(_launch(L, case, outs))
    assert all(o.bands_untouched() for o in outs), "the launch wrote outside its output"
    got = torch.cat([o.out.float().cpu() if case.out_f32 == 3 else from_nhwc(o.out) for o in outs], 1)
    assert torch.isfinite(got).all(), f"{int((~torch.isfinite(got)).sum())} elements not written"
    fig = CC.figure(got, case)
    print(f"{case.id} [{case.family}]: {fig:.3g} of the bound")
    assert fig <= 1.0, (case.id, fig)
    if case.code == 0:
        ref, _ = CC.reference(case)
        assert torch.allclose(got, ref.float(), **tol(0, ref.abs().max().item())), (got - ref.float()).abs().max()


@pytest.mark.parametrize("case", CC.REJECTED, ids=lambda c: c.id)
def test_dilated_16_channel_launch_is_refused_and_writes_nothing(case):
    """vs_conv2d_variant plans cout tile 16 for a dilated layer of fewer than 32 channels; launch_tile builds no such kernel"""
    L = lib()
    outs = _outputs(case)
    before = outs[0].buf.clone()
    with option(**dict(case.options)):
        assert CC.queried(L, case)[0] == case.plan
        rc = _launch(L, case, outs)
    assert rc != 0 and L.last_error()
    assert torch.equal(outs[0].buf.view(outs[0].bits), before.view(outs[0].bits))
