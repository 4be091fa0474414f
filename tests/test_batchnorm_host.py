"""The cases, references and bounds of tests/batchnorm_cases.py without a GPU: the float64 references against float64 F.batch_norm with
float64 autograd (1e-12 relative), the row-map restatement against the hand-written table, every case's bounds against float32 torch
on the CPU (the bound can be met and the reference is right), and the margin that keeps every element of a recomputed mask in the
comparison."""
import math

import numpy as np
import pytest
import torch

import batchnorm_cases as B

ANCHOR_CASES = [B.Case(r, c, code, fam) for (r, c) in ((2, 8), (37, 24), (263, 520), (700, 304)) for code in (0, 1) for fam in ("plain", "constant")]


def _held(figures, context):
    failed = []
    for label, ratio in figures:
        print(f"{context} {label}: {ratio:.3g} of the bound")
        if not ratio <= 1.0:
            failed.append((label, ratio))
    assert not failed, (context, failed)


def _rel(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


@pytest.mark.parametrize("shape", list(B.LAUNCHES), ids=lambda s: f"{s[0]}x{s[1]}")
def test_rowmap_restatement_selects_the_launch_of_the_table(shape):
    """(nblocks, iterations per block, trips, idle threads, empty blocks, rows of the last busy block, rows live in the last trip)"""
    rows, c = shape
    assert B.launch(rows, c) == B.LAUNCHES[shape]
    m = B.rowmap(rows, c)
    assert m.nblocks * m.rows_per_block >= rows and m.nblocks <= B.MAX_BLOCKS       # every row has a block
    assert m.nblocks <= 2048                                                           # the rows vs_bn_workspace holds


def test_table_reaches_what_the_issue_names():
    nblocks = {s: v[0] for s, v in B.LAUNCHES.items()}
    assert nblocks[(1025, 2048)] == 257 and nblocks[(33000, 64)] == 258            # the u = 1 lane of strided_sum2_f64 sees real rows
    assert B.LAUNCHES[(4100, 2048)][:3] == (1024, 5, 2) and B.LAUNCHES[(4100, 2048)][4] == 204 and B.LAUNCHES[(4100, 2048)][6] == 1
    assert B.LAUNCHES[(524800, 16)][:3] == (1024, 5, 2) and B.rowmap(524800, 16).rpb == 128
    assert 70 % B.rowmap(70, 48).rpb == 28 and B.rowmap(37, 24).rpb == 85 and B.rowmap(263, 520).cv == 65
    for c, rg in ((8, 64), (64, 8), (512, 1)):                                      # row groups of the inline sums: 256 / (2 c / 4)
        assert 256 // (2 * c // 4) == rg and 256 % (2 * c // 4) == 0
    assert 256 % (2 * 24 // 4) != 0                                                 # c = 24: the per-channel fallback


@pytest.mark.parametrize("case", ANCHOR_CASES, ids=lambda c: c.id)
def test_references_agree_with_float64_batch_norm_and_autograd(case):
    """every reference formula of the case module, fed float64 statistics, against F.batch_norm(training=True) + autograd in float64"""
    x, res, dy, _, gamma, beta, rm0, rv0 = B.inputs(case)
    ry, rdx, rdres, rdgamma, rdbeta, rrm, rrv = B.chained_reference(x, res, dy, gamma, beta, rm0, rv0)
    mean, var = B.ref_stats(x.double())
    invstd = 1 / torch.sqrt(var + B.f32(1e-5))
    mom, n = B.f32(0.1), case.rows
    assert _rel((1 - mom) * rm0.double() + mom * mean, rrm) < 1e-12
    assert _rel((1 - mom) * rv0.double() + mom * var * n / (n - 1), rrv) < 1e-12
    y, _ = B.apply_reference(x, res, 1, gamma, beta, mean, invstd, case.code)
    assert _rel(y, ry) < 1e-12
    g = B.masked_gradient(x, dy, y, "y", gamma, beta, mean, invstd)
    assert torch.equal(g, rdres)
    xhat = (x.double() - mean) * invstd
    dbeta, dgamma = g.sum(0), (g * xhat).sum(0)
    assert _rel(dbeta, rdbeta) < 1e-12 and _rel(dgamma, rdgamma) < 1e-12
    dx, _ = B.dx_reference(g, x, mean, invstd, gamma, dgamma, dbeta, n, case.code)
    assert _rel(dx, rdx) < 1e-11          # (1e-12 of the largest term: the three terms of dx cancel)
    # without a residual the recomputed mask is the mask of y
    y0, _ = B.apply_reference(x, None, 1, gamma, beta, mean, invstd, case.code)
    assert torch.equal(B.masked_gradient(x, dy, None, "recompute", gamma, beta, mean, invstd), dy.double() * (y0 > 0))


def test_one_row_takes_the_unbiased_guard():
    x, _, _, _, _, _, rm0, rv0 = B.inputs(B.Case(1, 8, 0))
    mean, invstd, rm, rv = B.float32_stages(B.Case(1, 8, 0))
    assert torch.equal(mean, x[0]) and torch.equal(invstd, torch.full((8,), float(np.float32(1 / math.sqrt(B.f32(1e-5))))))
    assert torch.allclose(rv.double(), 0.9 * rv0.double(), rtol=1e-6)              # var 0, not 0 / 0
    _held(B.stats_figures(x, 1e-5, 0.1, rm0, rv0, mean, invstd, rm, rv, B.rowmap(1, 8)), "1x8")


@pytest.mark.parametrize("case", B.TWO_SWEEP_CASES, ids=lambda c: c.id)
def test_float32_torch_stays_within_every_bound(case):
    """float32 torch on the CPU in the device's place.  The |mean - K| families (offset, outlier-K, and constant, whose constant channels
    have x - K = 0 and a bound of one rounding) are exempt from that for the statistics: their bounds are on sums of x - K, torch sums x
    itself and (offset: |mean| = 6000 std) cannot meet them; for those families only, a float32 NumPy restatement of the shifted sums
    stands in.  Shapes above a million elements run one branch of each stage here."""
    x, res, dy, y_ties, gamma, beta, rm0, rv0 = B.inputs(case)
    m, code = B.rowmap(case.rows, case.c), case.code
    big = case.rows * case.c > 1 << 20
    shifted = case.family in ("offset", "outlier-K", "constant")
    for eps, mom in (B.EPS_MOM[:1] if big else B.EPS_MOM):
        mean, invstd, rm, rv = B.float32_stages(case, eps, mom, shifted)
        _held(B.stats_figures(x, eps, mom, rm0, rv0, mean, invstd, rm, rv, m), f"{case.id} eps={eps:g}")
    mean, invstd, _, _ = B.float32_stages(case, 1e-5, 0.1, shifted)
    for relu, r in (((1, res),) if big else ((0, None), (0, res), (1, None), (1, res))):
        y = B.float32_apply(x, r, relu, gamma, beta, mean, invstd, code)
        _held(B.apply_figures(f"apply relu={relu} res={int(r is not None)}", x, r, relu, gamma, beta, mean, invstd, y, code), case.id)
    if not case.backward:
        return
    y_in = y_ties if y_ties is not None else B.rounded(B.apply_reference(x, res, 1, gamma, beta, mean, invstd, code)[0].float(), code)
    if y_ties is not None:
        assert (y_ties == 0).float().mean() > 0.5 and (y_ties > 0).any()
    modes = ("y",) if big else (("none", "y", "recompute") if case.recompute else ("none", "y"))
    for mode in modes:
        g = B.masked_gradient(x, dy, y_in, mode, gamma, beta, mean, invstd)
        dx, dgamma, dbeta = B.float32_bwd(g, x, mean, invstd, gamma, code)
        _held(B.bwd_sums_figures(mode, g, x, mean, invstd, dgamma, dbeta, m), case.id)
        _held(B.dx_figures(mode, g, x, mean, invstd, gamma, dgamma, dbeta, dx, B.rounded(g.float(), code), code), case.id)
        assert torch.isfinite(dx).all()


@pytest.mark.parametrize("case", [c for c in B.TWO_SWEEP_CASES if c.recompute], ids=lambda c: c.id)
def test_recomputed_mask_keeps_its_margin(case):
    """min |pre-activation| >= 1e-3 under the float64 statistics, for every case whose mask is recomputed: no element is left out"""
    x, _, _, _, gamma, beta, _, _ = B.inputs(case)
    assert B.preactivation(x, gamma, beta).abs().min().item() >= B.MARGIN
    assert torch.equal(x, B.rounded(x, case.code))


@pytest.mark.parametrize("case", B.CHAINED_CASES, ids=lambda c: c.id)
def test_chained_bounds_hold_for_float32_torch(case):
    x, res, dy, gamma, beta, rm0, rv0 = B.chained_inputs(case)
    mean, var = x.mean(0), x.var(0, unbiased=False)
    invstd = 1 / torch.sqrt(var + 1e-5)
    rm, rv = 0.9 * rm0 + 0.1 * mean, 0.9 * rv0 + 0.1 * var * (case.rows / (case.rows - 1))
    y = B.float32_apply(x, res, 1, gamma, beta, mean, invstd, case.code)
    g = dy * (y > 0)
    dx, dgamma, dbeta = B.float32_bwd(g, x, mean, invstd, gamma, case.code)
    _held(B.chained_figures(case, (mean, invstd, rm, rv, y, dx, g, dgamma, dbeta)), case.id)


@pytest.mark.parametrize("c", B.FOLD_C)
def test_fold_bound_holds_for_float32_torch(c):
    gamma, beta, rm, rv = B.fold_inputs(c)
    assert (rv == 0).any() and (rv > 0).any()
    for eps in (1e-5, 1e-3):
        s = gamma / torch.sqrt(rv + np.float32(eps))
        _held(B.fold_figures(gamma, beta, rm, rv, eps, s, beta - rm * s), f"fold c={c} eps={eps:g}")


@pytest.mark.parametrize("nparts", B.INLINE_NPARTS)
def test_rows_handed_to_the_inline_sweeps(nparts):
    """unequal shares, some negative, that add up to the sums; the statistics defined from the fp32 rows are met to within 1 ulp by a
    float64 sum in another order; the bins add up exactly, hold negative entries, and some channels have a negative mean"""
    c, rows = 64, 300
    x, _, _, _, rm0, rv0, _, _, _ = B.inline_inputs(c, rows, 0)
    w = B.shares(nparts, nparts + c)
    assert abs(w.sum() - 1) < 1e-12 and (nparts < 5 or (w < 0).any()) and (nparts == 1 or np.ptp(w) > 0.5 / nparts)
    s, q = x.double().sum(0), (x.double() ** 2).sum(0)
    assert (s < 0).any() and (s > 0).any()
    part = B.split_rows(s, q, nparts, nparts + c)
    assert part.shape == (nparts, 2, c) and part.dtype == torch.float32
    want = B.defined_stats(part[:, 0].double().sum(0), part[:, 1].double().sum(0), rows, 1e-5, 0.1, rm0, rv0)
    other = B.defined_stats(part[:, 0].double().flip(0).cumsum(0)[-1], part[:, 1].double().flip(0).cumsum(0)[-1], rows, 1e-5, 0.1, rm0, rv0)
    _held(B.published_figures("another order", want, tuple(t.float() for t in other)), f"parts={nparts}")
    assert torch.allclose(want[0], x.double().mean(0), atol=1e-5) and torch.allclose(want[1], 1 / torch.sqrt(x.double().var(0, unbiased=False) + 1e-5), rtol=1e-3)
    if nparts in B.BINS_NB:
        bins, tot = B.split_bins(s, q, nparts, nparts + c)
        assert bins.dtype == torch.int64 and torch.equal(bins.sum(0), tot) and (nparts == 1 or (bins < 0).any()) and (tot[0] < 0).any()
        assert torch.allclose(tot[0].double() / 2 ** 24, s, atol=2.0 ** -24) and torch.allclose(tot[1].double() / 2 ** 16, q, atol=2.0 ** -16)


def test_inline_shapes_run_one_and_three_workgroups():
    for c in sorted(set(B.INLINE_C + B.BINS_C)):
        assert B.rowmap(B.inline_rows(c, False), c).nblocks == 1 and B.rowmap(B.inline_rows(c, True), c).nblocks == 3
        assert B.inline_rows(c, True) % B.rowmap(1, c).rpb == 1 % B.rowmap(1, c).rpb       # ragged last iteration (but for one row per iteration)


@pytest.mark.parametrize("h,cin,cout", [(8, 512, 512), (16, 256, 256)])
def test_epilogue_variance_bound_holds_for_a_float32_product(h, cin, cout):
    """the inputs of the non-zero-mean ring cases: rho from about 0 to about 32 across the output channels, and float32 accumulators
    with float32 sums (torch on the CPU) in the device's place stay within the bound, which grows like 1 + rho^2"""
    x, wt, ref = B.ring_inputs(h, h, cin, cout)
    assert torch.equal(x, B.rounded(x, 1)) and torch.equal(wt, B.rounded(wt, 1)) and (x >= 0).all()
    a = torch.nn.functional.unfold(x, 3, padding=1).transpose(1, 2).reshape(-1, 9 * cin) @ wt.reshape(cout, -1).t()
    figures, curve, _ = B.ring_variance_figures(h, cin, cout, a.sum(0).double(), (a * a).sum(0).double(), 32, False)
    _held(figures, f"{h}x{h} {cin}->{cout}")
    rho, bound = curve[:, 0], curve[:, 3]
    assert rho.min() < 2 and rho.max() > 16
    assert bound[rho.argmax()] > 10 * bound[rho.argmin()]        # relative to the variance, the bound grows with rho
