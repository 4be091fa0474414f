"""-m gpu: the data-movement kernels of csrc/pool.hip through the C ABI against the plain CPU references of tests/pool_cases.py - the
max-pool forward (values bit for bit, the stored arg-max codes against a scan in the kernel's documented order) and backward (a float64
scatter by the stored codes), vs_channel_slice (copy and accumulate, offsets, the channels around the slice), the backward of the nearest
upsampling, zero stuffing and the two pixel shuffles - at one window, at channel counts that are no multiple of 64, and, for the max-pool
and the channel slice, at a size where the grid-stride loop of a launch capped at 8192 workgroups takes a second trip."""
import pytest
import torch

import pool_cases as PC
from conv_cases import DT, worst
from hip_helpers import DEV, lib, rounded, sync, tdtype

pytestmark = pytest.mark.gpu
CODES = [0, 1, 2]
POOL_SHAPES = [(1, 2, 2, 8), (2, 6, 10, 24), (3, 16, 24, 40)]          # (n, h, w, c): one window; ragged against nothing, c no multiple of 64
MOVE_SHAPES = [(2, 3, 5, 8), (2, 3, 5, 40)]


def _dev(t, code):
    return t.to(tdtype(code)).contiguous().to(DEV)


def _nan(shape, code):
    return torch.full(shape, float("nan"), device=DEV, dtype=tdtype(code))


def _pool_input(kind, shape, code, g):
    n, h, w, c = shape
    if kind == "relu":              # ReLU output: ties at 0
        return rounded(torch.randn(n, h, w, c, generator=g), code).relu()
    if kind == "constant":
        return torch.full((n, h, w, c), 1.5)
    return -rounded(torch.rand(n, h, w, c, generator=g) + 0.25, code)      # all negative: padding must never win


@pytest.mark.parametrize("code", CODES, ids=lambda c: DT[c])
@pytest.mark.parametrize("shape", POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", ["relu", "constant", "negative"])
def test_maxpool_forward_codes_and_backward(code, shape, kind):
    L = lib()
    n, h, w, c = shape
    g = torch.Generator().manual_seed(1000 * code + h * w + c)
    x = _pool_input(kind, shape, code, g)
    y_scan, codes = PC.maxpool_scan(x.numpy())
    assert torch.equal(y_scan, PC.maxpool_torch(x))                  # the two CPU references agree on the values
    xd = _dev(x, code)
    yd = _nan((n, h // 2, w // 2, c), code)
    idx = torch.full((n, h // 2, w // 2, c), 255, device=DEV, dtype=torch.uint8)
    L.check(L.lib.vs_maxpool_fwd(code, L.ptr(xd), L.ptr(yd), L.ptr(idx), n, h, w, c, None))
    sync()
    assert torch.equal(PC.bits(yd.cpu()), PC.bits(y_scan.to(tdtype(code)))), "y differs from F.max_pool2d"
    got_codes = idx.cpu()
    assert torch.equal(got_codes, codes), f"{int((got_codes != codes).sum())} arg-max codes differ from the (kh, kw) scan with strict >"
    if kind == "constant":
        assert bool((got_codes[:, 0, 0] == 4).all())                 # the top-left window: its first tap inside the image is the centre
    if kind == "negative":
        assert bool((yd.float().cpu() < 0).all())
    # without the codes the forward stores the same values
    y2 = _nan((n, h // 2, w // 2, c), code)
    L.check(L.lib.vs_maxpool_fwd(code, L.ptr(xd), L.ptr(y2), None, n, h, w, c, None))
    sync()
    assert torch.equal(PC.bits(y2.cpu()), PC.bits(yd.cpu()))
    dy = rounded(torch.randn(n, h // 2, w // 2, c, generator=g), code)
    base = rounded(torch.randn(n, h, w, c, generator=g), code)
    dyd = _dev(dy, code)
    for accumulate in (0, 1):
        dx = _dev(base, code) if accumulate else _nan((n, h, w, c), code)
        L.check(L.lib.vs_maxpool_bwd(code, L.ptr(dyd), L.ptr(idx), L.ptr(dx), accumulate, n, h, w, c, None))
        sync()
        ref, mag = PC.maxpool_scatter(dy, got_codes, h, w, base if accumulate else None)
        fig = worst((dx.cpu().double() - ref).abs(), PC.summed_bound(ref, mag, 4, code))
        print(f"maxpool_bwd {DT[code]} {shape} {kind} accumulate={accumulate}: {fig:.3g} of the bound")
        assert fig <= 1.0, fig


def test_maxpool_grid_stride_second_trip():
    """bf16, 2 x 730 x 730 x 64: 2 131 600 items, more than 8192 workgroups x 256 threads, so the last items of the forward and of the
    backward are reached only by the loop's second trip.  Small integers: every value, and every sum of up to four gradients, is exact
    in bf16, so both directions are compared bit for bit with one F.max_pool2d call and its autograd gradient (which routes to the first
    maximum in scan order, like the stored codes)."""
    L = lib()
    code, n, h, w, c = 1, 2, 730, 730, 64
    assert n * (h // 2) * (w // 2) * (c // 8) > PC.GRID_ITEMS
    g = torch.Generator().manual_seed(730)
    x = torch.randint(-100, 101, (n, h, w, c), generator=g, dtype=torch.int8).float()
    dy = torch.randint(1, 9, (n, h // 2, w // 2, c), generator=g, dtype=torch.int8).float()
    xg = x.permute(0, 3, 1, 2).requires_grad_()
    y = torch.nn.functional.max_pool2d(xg, 3, 2, 1)
    y.backward(dy.permute(0, 3, 1, 2))
    y_ref, dx_ref = y.detach().permute(0, 2, 3, 1), xg.grad.permute(0, 2, 3, 1)
    xd, dyd = _dev(x, code), _dev(dy, code)
    yd, dx = _nan(dy.shape, code), _nan(x.shape, code)
    idx = torch.full(dy.shape, 255, device=DEV, dtype=torch.uint8)
    L.check(L.lib.vs_maxpool_fwd(code, L.ptr(xd), L.ptr(yd), L.ptr(idx), n, h, w, c, None))
    L.check(L.lib.vs_maxpool_bwd(code, L.ptr(dyd), L.ptr(idx), L.ptr(dx), 0, n, h, w, c, None))
    sync()
    assert torch.equal(yd.cpu(), y_ref.to(torch.bfloat16))
    assert int(idx.max()) <= 8
    assert torch.equal(dx.cpu(), dx_ref.to(torch.bfloat16))


SLICES = [(5, 24, 8, 40, 16, 16), (7, 8, 0, 8, 0, 8)]      # (rows, c_src, src_off, c_dst, dst_off, c)


def _slice_case(code, case, accumulate):
    """dst starts as NaNs of distinct payloads (the slice itself as data when accumulating); afterwards the slice holds src's slice, or
    (src.float() + dst.float()).to(T), and every other channel its old bit pattern"""
    rows, c_src, src_off, c_dst, dst_off, c = case
    L = lib()
    T = tdtype(code)
    g = torch.Generator().manual_seed(rows + 7 * code + accumulate)
    src = rounded(torch.randn(rows, c_src, generator=g), code).to(T)
    dst = PC.nan_payloads((rows, c_dst), code).clone() if c_dst > c else torch.full((rows, c_dst), float("nan"), dtype=T)
    before = rounded(torch.randn(rows, c, generator=g), code).to(T)
    if accumulate:
        dst[:, dst_off:dst_off + c] = before
    want = dst.clone()
    piece = src[:, src_off:src_off + c]
    want[:, dst_off:dst_off + c] = (piece.float() + before.float()).to(T) if accumulate else piece
    sd, dd = src.to(DEV), dst.to(DEV)
    L.check(L.lib.vs_channel_slice(code, L.ptr(sd), c_src, src_off, L.ptr(dd), c_dst, dst_off, c, rows, accumulate, None))
    sync()
    assert torch.equal(PC.bits(dd.cpu()), PC.bits(want)), "the slice, or the channels around it, differ in their bit patterns"
    assert torch.equal(PC.bits(sd.cpu()), PC.bits(src))


@pytest.mark.parametrize("code", CODES, ids=lambda c: DT[c])
@pytest.mark.parametrize("case", SLICES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("accumulate", [0, 1])
def test_channel_slice_copy_and_accumulate(code, case, accumulate):
    _slice_case(code, case, accumulate)


@pytest.mark.parametrize("accumulate", [0, 1])
def test_channel_slice_grid_stride_second_trip(accumulate):
    """262 149 rows x 8 groups of 8 channels = 2 097 192 items: the last 40 are reached only by the loop's second trip"""
    case = (262149, 64, 0, 64, 0, 64)
    assert case[0] * (case[5] // 8) > PC.GRID_ITEMS
    _slice_case(1, case, accumulate)


@pytest.mark.parametrize("code", CODES, ids=lambda c: DT[c])
def test_channel_slice_no_rows_and_refused_launches(code):
    L = lib()
    src = torch.ones(5, 24, dtype=tdtype(code), device=DEV)
    dst = PC.nan_payloads((5, 40), code).to(DEV)
    before = PC.bits(dst.cpu())
    L.check(L.lib.vs_channel_slice(code, L.ptr(src), 24, 8, L.ptr(dst), 40, 16, 16, 0, 0, None))          # rows = 0
    sync()
    assert torch.equal(PC.bits(dst.cpu()), before)
    for c_src, src_off, c_dst, dst_off, c in ((24, 4, 40, 16, 16), (24, 8, 40, 4, 16), (24, 16, 40, 16, 16), (24, 8, 40, 32, 16), (24, 8, 40, 16, 0)):
        rc = L.lib.vs_channel_slice(code, L.ptr(src), c_src, src_off, L.ptr(dst), c_dst, dst_off, c, 5, 0, None)
        sync()
        assert rc != 0 and "channel_slice" in L.last_error(), (c_src, src_off, c_dst, dst_off, c)
        assert torch.equal(PC.bits(dst.cpu()), before)


@pytest.mark.parametrize("code", CODES, ids=lambda c: DT[c])
@pytest.mark.parametrize("shape", MOVE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_upsample2x_bwd_is_the_fp32_chain_bit_for_bit(code, shape):
    L = lib()
    n, h, w, c = shape
    g = torch.Generator().manual_seed(31 + c + code)
    dy = rounded(torch.randn(n, 2 * h, 2 * w, c, generator=g), code)
    dyd, dx = _dev(dy, code), _nan(shape, code)
    L.check(L.lib.vs_upsample2x_bwd(code, L.ptr(dyd), L.ptr(dx), n, h, w, c, None))
    sync()
    assert torch.equal(PC.bits(dx.cpu()), PC.bits(PC.upsample2x_bwd_chain(dy).to(tdtype(code))))


@pytest.mark.parametrize("code", CODES, ids=lambda c: DT[c])
@pytest.mark.parametrize("shape", MOVE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_zero_stuffing_and_pixel_shuffles_are_exact_permutations(code, shape):
    L = lib()
    n, h, w, c = shape
    g = torch.Generator().manual_seed(57 + c + code)
    T = tdtype(code)
    x = rounded(torch.randn(n, h, w, c, generator=g), code).to(T)
    xd, y = x.to(DEV), _nan((n, 2 * h, 2 * w, c), code)
    L.check(L.lib.vs_zero_stuff2x(code, L.ptr(xd), L.ptr(y), n, h, w, c, None))
    sync()
    assert torch.equal(PC.bits(y.cpu()), PC.bits(PC.zero_stuffed(x)))
    x4 = rounded(torch.randn(n, h, w, 4 * c, generator=g), code).to(T)
    x4d, up = x4.to(DEV), _nan((n, 2 * h, 2 * w, c), code)
    L.check(L.lib.vs_depth_to_space2(code, L.ptr(x4d), L.ptr(up), n, h, w, c, None, None, None, 0, None))
    sync()
    assert torch.equal(PC.bits(up.cpu()), PC.bits(PC.depth_to_space(x4)))
    back = _nan((n, h, w, 4 * c), code)
    L.check(L.lib.vs_space_to_depth2(code, L.ptr(up), L.ptr(back), n, h, w, c, None))
    sync()
    assert torch.equal(PC.bits(back.cpu()), PC.bits(x4)), "space_to_depth2 after depth_to_space2 is not the identity"
    assert torch.equal(PC.bits(PC.space_to_depth(PC.depth_to_space(x4))), PC.bits(x4))
    # the shuffle's epilogue: + bias, * scale + shift, ReLU
    bias, scale, shift = torch.randn(c, generator=g), torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g)
    bd, scd, shd = bias.to(DEV), scale.to(DEV), shift.to(DEV)
    for relu in (0, 1):
        out = _nan((n, 2 * h, 2 * w, c), code)
        L.check(L.lib.vs_depth_to_space2(code, L.ptr(x4d), L.ptr(out), n, h, w, c, L.ptr(bd), L.ptr(scd), L.ptr(shd), relu, None))
        sync()
        ref, bound = PC.depth_to_space_epilogue(x4.float(), bias, scale, shift, relu, code)
        fig = worst((out.cpu().double() - ref).abs(), bound)
        print(f"depth_to_space2 epilogue {DT[code]} {shape} relu={relu}: {fig:.3g} of the bound")
        assert fig <= 1.0, fig
