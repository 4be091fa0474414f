"""-m gpu: every kernel form the launches of csrc/stem.hip can select (tests/stem_cases.py: the fp32-arithmetic forward with its fp32, bf16 and
fp16 stores, the bf16 MFMA forward with and without the statistics bins, the fp32-arithmetic and the bf16 MFMA weight gradient), at the
three shapes of the table, one small launch each through the C ABI against the float64 CPU reference of the same operands: the launch
writes every element of its output (prefilled with NaN) and nothing in the guard bands around it and around a workspace of exactly the
queried size, the error stays within the per-element bound derived in stem_cases.py, and a second launch gives the same bits.  The bins
rows also store z bit for bit as vs_stem_fwd does.  The launches the table says must be refused return an error and write nothing."""
import pytest
import torch

import stem_cases as SC
from hip_helpers import DEV, from_nhwc, lib, option, sync, tdtype, to_nhwc

pytestmark = pytest.mark.gpu
SENTINEL = -77.0
BAND = 256                # elements on either side


class Guarded:
    """`count` elements of NaN inside a larger buffer, SENTINEL in a band before and after them"""
    def __init__(self, count, dtype=torch.float32):
        self.buf = torch.full((count + 2 * BAND,), SENTINEL, device=DEV, dtype=dtype)
        self.out = self.buf[BAND:BAND + count]
        self.out.fill_(float("nan"))
        self.start = self.bits()

    def bands_untouched(self):
        edge = torch.cat([self.buf[:BAND], self.buf[-BAND:]])
        return bool((edge == SENTINEL).all())

    def bits(self):
        return self.buf.view(torch.int16 if self.buf.element_size() == 2 else torch.int32).clone()


def _device_inputs(case):
    x, w, scale, shift, dy = SC.inputs(case)
    dev = lambda t: None if t is None else t.contiguous().to(DEV)
    return dev(x), dev(w.reshape(64, 49)), dev(scale), dev(shift), (to_nhwc(dy, case.code) if dy is not None else None)


def _run(L, case, ops):
    """one launch of the row into fresh guarded buffers: (output on the CPU laid out as the reference, raw output bits, bins or None)"""
    xd, wd, scd, shd, dyd = ops
    s = case.shape
    out = Guarded(SC.out_elems(case), torch.float32 if case.is_wgrad else tdtype(case.code))
    ws = bins = None
    asked = 0
    if case.is_wgrad:
        asked = L.lib.vs_stem_wgrad_workspace(s.n, s.h, s.w)
        assert asked % 4 == 0
        ws = Guarded(asked // 4)
    if case.form == "fwd-bins":
        bins = torch.zeros((case.nb, 2, 64), dtype=torch.int64, device=DEV)
    L.check(SC.launch(L, case, xd, wd, out.out, scale=scd, shift=shd, dy=dyd, ws=None if ws is None else ws.out, ws_bytes=asked, bins=bins))
    sync()
    assert out.bands_untouched(), "the launch wrote outside its output"
    assert ws is None or ws.bands_untouched(), "the launch wrote outside the workspace it asked for"
    raw = out.out.clone()
    got = raw.cpu().view(64, 49) if case.is_wgrad else from_nhwc(raw.view(s.n, case.hout, case.wout, 64))
    return got, raw, (None if bins is None else bins.cpu())


@pytest.mark.parametrize("case", SC.CASES, ids=lambda c: c.id)
def test_stem_launch_within_the_per_element_bound(case):
    L = lib()
    ops = _device_inputs(case)
    got, raw, bins = _run(L, case, ops)
    again, raw2, bins2 = _run(L, case, ops)
    assert torch.isfinite(got).all(), f"{int((~torch.isfinite(got)).sum())} elements not written"
    if case.form == "fwd-bins":
        scales = (L.lib.vs_stat_scale(0), L.lib.vs_stat_scale(1))
        fig = SC.figure(SC.bins_totals(bins, scales), case)
        ref, bound = SC.stored_reference(case)
        zfig = SC.figure_against(got, ref, bound)
        print(f"{case.id} [{case.form}]: totals {fig:.3g} of the bound, stored z {zfig:.3g} of the bound")
        assert fig <= 1.0 and zfig <= 1.0, (case.id, fig, zfig)
        # the workgroups add to rows blockIdx & (nb - 1): with 16 or more of them no row stays empty
        assert SC.workgroups(case) < case.nb or bool(bins[:, 1].sum(1).ne(0).all())
        plain = torch.full_like(raw, float("nan"))
        with option(**dict(case.options)):
            L.check(L.lib.vs_stem_fwd(case.code, L.ptr(ops[0]), L.ptr(ops[1]), None, None, 0, L.ptr(plain), case.shape.n, case.shape.h, case.shape.w, None))
        sync()
        assert torch.equal(raw.view(torch.int16), plain.view(torch.int16)), "the bins launch stores another z than vs_stem_fwd"
        assert torch.equal(bins, bins2), "two launches of the same operands leave different bins"
    else:
        fig = SC.figure(got, case)
        print(f"{case.id} [{case.form}]: {fig:.3g} of the bound")
        assert fig <= 1.0, (case.id, fig)
    view = torch.int16 if raw.element_size() == 2 else torch.int32
    assert torch.equal(raw.view(view), raw2.view(view)), "two launches of the same operands differ"


@pytest.mark.parametrize("case", SC.REFUSED, ids=lambda c: c.id)
def test_refused_launch_returns_an_error_and_writes_nothing(case):
    L = lib()
    s = case.shape
    xd, wd, _, _, dyd = _device_inputs(case)
    out = Guarded(SC.out_elems(case), torch.float32 if case.is_wgrad else tdtype(case.code))
    asked = L.lib.vs_stem_wgrad_workspace(s.n, s.h, s.w)
    ws = Guarded(asked // 4) if case.is_wgrad else None
    bins = torch.zeros((16, 2, 64), dtype=torch.int64, device=DEV) if case.form == "fwd-bins" else None
    rc = SC.launch(L, case, xd, wd, out.out, dy=dyd, ws=None if ws is None else ws.out, ws_bytes=asked - case.ws_short, bins=bins)
    sync()
    assert rc != 0 and L.last_error()
    assert torch.equal(out.bits(), out.start) and (ws is None or torch.equal(ws.bits(), ws.start)) and (bins is None or not bool(bins.any()))
