"""What tests/test_hip_pool_moves.py compares the data-movement kernels of csrc/pool.hip with: plain CPU references of the same operation on
NHWC tensors.  Pure moves are compared bit for bit; arithmetic of a fixed order bit for bit against the same order in fp32 on the CPU;
where the compiler may or may not fuse, or the order is the kernel's own, a counted-rounding bound (U, gamma, STORE of
tests/conv_cases.py) on the float64 reference.

grid_for caps a launch at 8192 workgroups of 256 threads, one item (8 channels) a thread a trip: a second trip of the grid-stride loop
runs only above GRID_ITEMS = 2 097 152 items."""
import numpy as np
import torch
import torch.nn.functional as F

from conv_cases import STORE, U, gamma
from hip_helpers import tdtype

GRID_ITEMS = 8192 * 256


def bits(t):
    """the bit patterns of a tensor as integers of its element size"""
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def nan_payloads(shape, code):
    """a tensor of the dtype whose every element is a NaN, with payloads that differ between neighbours"""
    count = int(np.prod(shape))
    i = torch.arange(count, dtype=torch.int64)
    if code == 0:
        pat = (0x7FC00000 + 1 + i % 0x3FFFFF).to(torch.int32)
    elif code == 1:
        pat = (0x7FC0 + 1 + i % 63 + (i // 63 % 2) * 0x8000)               # quiet NaNs of either sign, 6 payload bits
        pat = torch.where(pat >= 0x8000, pat - 0x10000, pat).to(torch.int16)
    else:
        pat = (0x7E00 + 1 + i % 511 + (i // 511 % 2) * 0x8000)
        pat = torch.where(pat >= 0x8000, pat - 0x10000, pat).to(torch.int16)
    out = pat.view(tdtype(code)).view(shape)
    assert bool(torch.isnan(out).all())
    return out


# ---- max-pool 3 x 3, stride 2, padding 1 --------------------------------------------------------------------------------------------
def maxpool_scan(x):
    """(y, codes) of an NHWC fp32 array by the scan the kernel documents: taps in (kh, kw) order, a strict > against the best so far,
    starting from -inf with code 0; padding is never looked at"""
    x = np.asarray(x, dtype=np.float32)
    n, h, w, c = x.shape
    ho, wo = h // 2, w // 2
    xp = np.full((n, h + 2, w + 2, c), -np.inf, dtype=np.float32)
    xp[:, 1:-1, 1:-1] = x
    best = np.full((n, ho, wo, c), -np.inf, dtype=np.float32)
    code = np.zeros((n, ho, wo, c), dtype=np.uint8)
    for kh in range(3):
        for kw in range(3):
            v = xp[:, kh:kh + 2 * ho:2, kw:kw + 2 * wo:2]
            m = v > best
            best = np.where(m, v, best)
            code[m] = kh * 3 + kw
    return torch.from_numpy(best), torch.from_numpy(code)


def maxpool_torch(x):
    """F.max_pool2d(3, 2, 1) of an NHWC fp32 tensor, NHWC"""
    return F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).contiguous()


def maxpool_scatter(dy, codes, h, w, base=None):
    """float64 (reference, sum of |terms|) of the backward: every output pixel's gradient goes to the input pixel its stored code names;
    base: what dx held before an accumulating launch.  NHWC."""
    n, ho, wo, c = dy.shape
    ref = torch.zeros(n, h + 1, w + 1, c, dtype=torch.float64)          # input row hi at index hi + 1
    mag = torch.zeros_like(ref)
    d = dy.double()
    for k in range(9):
        kh, kw = divmod(k, 3)
        part = torch.where(codes == k, d, torch.zeros_like(d))
        ref[:, kh:kh + 2 * ho:2, kw:kw + 2 * wo:2] += part
        mag[:, kh:kh + 2 * ho:2, kw:kw + 2 * wo:2] += part.abs()
    ref, mag = ref[:, 1:, 1:], mag[:, 1:, 1:]
    assert not bool(torch.where(codes > 8, 1, 0).any())
    if base is not None:
        ref, mag = ref + base.double(), mag + base.double().abs()
    return ref.contiguous(), mag.contiguous()


def summed_bound(ref, mag, m, code):
    """a sum in which no term meets more than m fp32 roundings, stored in the dtype: gamma_m sum |terms| + half an ulp of the store"""
    err = gamma(m) * mag
    u, tiny = STORE[code]
    return err + (u * (ref.abs() + err)).clamp_min(tiny)


# ---- moves ----------------------------------------------------------------------------------------------------------------------------
def upsample2x_bwd_chain(dy):
    """the kernel's order in fp32: (((0 + v00) + v01) + v10) + v11 over the 2 x 2 block; dy NHWC fp32"""
    s = torch.zeros_like(dy[:, 0::2, 0::2])
    for a in range(2):
        for b in range(2):
            s = s + dy[:, a::2, b::2]
    return s


def zero_stuffed(x):
    n, h, w, c = x.shape
    y = torch.zeros(n, 2 * h, 2 * w, c, dtype=x.dtype)
    y[:, 0::2, 0::2] = x
    return y


def depth_to_space(x):
    """y[n][2i+a][2j+b][k] = x[n][i][j][(2a+b) c + k]"""
    n, h, w, c4 = x.shape
    c = c4 // 4
    return x.view(n, h, w, 2, 2, c).permute(0, 1, 3, 2, 4, 5).reshape(n, 2 * h, 2 * w, c).contiguous()


def space_to_depth(y):
    """x[n][i][j][(2a+b) c + k] = y[n][2i+a][2j+b][k]"""
    n, h2, w2, c = y.shape
    return y.view(n, h2 // 2, 2, w2 // 2, 2, c).permute(0, 1, 3, 2, 4, 5).reshape(n, h2 // 2, w2 // 2, 4 * c).contiguous()


def depth_to_space_epilogue(x, bias, scale, shift, relu, code):
    """float64 (reference, bound) of vs_depth_to_space2 with every part of its epilogue: + bias, * scale, + shift - one rounding each,
    charged on the magnitude that flows through it (a fused multiply-add rounds once; two are charged) - ReLU, the store"""
    val = depth_to_space(x).double() + bias.double()
    err = U * val.abs()
    val, err = val * scale.double(), err * scale.double().abs()
    err = err + U * (val.abs() + err)
    val = val + shift.double()
    err = err + U * (val.abs() + err)
    if relu:
        val = val.clamp_min(0)
    u, tiny = STORE[code]
    return val, err + (u * (val.abs() + err)).clamp_min(tiny)
