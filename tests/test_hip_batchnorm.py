"""-m gpu: every BatchNorm kernel form of csrc/norm.hip against the float64 references and the derived bounds of
tests/batchnorm_cases.py - the two-launch statistics, the plain apply, the two-sweep backward (mask from y, recomputed, none), the
fold; and, through the vs_bn_*_from_* test seams, the inline apply from fp32 partial rows and from fixed-point bins, the partial-row
finalise and the inline backward, each under bn_prefetch 0 and 1.  Shapes are the smallest that select each launch (grid above 256
blocks, the 1024-block cap with its second trip and empty blocks, idle threads, ragged trips); every output starts as NaN.  The cases,
the launch each selects and the derivation of every bound are in the case module; tests/test_batchnorm_host.py checks them without a
GPU.  A figure is measured error over bound: at most 1."""
import pytest

import batchnorm_cases as B

pytestmark = pytest.mark.gpu


def _held(figures, context):
    failed = []
    for label, ratio in figures:
        print(f"{context} {label}: {ratio:.3g} of the bound")
        if not ratio <= 1.0:
            failed.append((label, ratio))
    assert not failed, (context, failed)


@pytest.mark.parametrize("case", B.TWO_SWEEP_CASES, ids=lambda c: c.id)
def test_two_sweep_operators_against_float64(case):
    """vs_bn_stats (running statistics null / not null, both (eps, momentum)), vs_bn_apply (relu x residual), vs_bn_bwd and
    vs_bn_bwd_recompute (mask none / y / recomputed, dres absent / present), each stage judged from the device state before it.
    The statistics bounds are on sums of x - K (K = row 0): the outlier-K family documents their growth with (mean - K)^2, the offset
    family is what the shift exists for; constant channels give invstd = float32(1 / sqrt(eps)) to the bit and finite dx; the ties
    family hands the backward a y that is mostly exact zeros (the mask y > 0 is strict)."""
    _held(B.two_sweep_figures(case), case.id)


@pytest.mark.parametrize("case", B.CHAINED_CASES, ids=lambda c: c.id)
def test_chained_stages_against_float64_batch_norm_and_autograd(case):
    """statistics -> apply (residual, relu) -> backward with the device's own y, end to end against F.batch_norm + autograd in float64,
    the stage bounds with the earlier stages' errors carried forward"""
    _held(B.chained_figures(case, B.chained_device(case)), case.id)


@pytest.mark.parametrize("eps", [1e-5, 1e-3])
@pytest.mark.parametrize("c", B.FOLD_C)
def test_fold_against_float64(c, eps):
    """vs_bn_fold with running_var down to exactly 0"""
    _held(B.fold_device(c, eps), f"fold c={c} eps={eps:g}")


def test_inline_rows_option_has_the_value_the_cases_assume():
    assert B._L().lib.vs_get_option(b"bn_inline_rows") == 64


@pytest.mark.parametrize("case", B.PARTIALS_CASES, ids=lambda c: c.id)
def test_inline_apply_from_partial_rows(case):
    """vs_bn_apply_from_partials: mean, invstd and the running statistics (exactly one momentum step: workgroup 0 alone publishes)
    within 1 ulp of their float64 definition from the fp32 rows handed in; y within the apply bound; same bits with and without prefetch"""
    _held(B.inline_forward_figures(case, "partials"), case.id)


@pytest.mark.parametrize("case", B.BINS_CASES, ids=lambda c: c.id)
def test_inline_apply_from_bins(case):
    """vs_bn_apply_from_bins: signed 64-bit bins with negative rows and negative channel sums, both bin-sum branches (2 c <= 256 and
    above), stat_rows = 2 rows in two cases"""
    _held(B.inline_forward_figures(case, "bins"), case.id)


@pytest.mark.parametrize("source", ["partials", "bins"])
@pytest.mark.parametrize("c", [64, 1024])
def test_inline_apply_without_running_statistics_relu_or_residual(c, source):
    _held(B.inline_null_running_figures(c, source), f"c={c} {source}")


@pytest.mark.parametrize("c", [8, 24, 520])
@pytest.mark.parametrize("nparts", B.FINALIZE_NPARTS)
def test_finalize_partials(nparts, c):
    """vs_bn_finalize_partials: 257 and 1100 rows reach the second to fourth row a thread of the fp64 strided sum loads per trip"""
    _held(B.finalize_figures(nparts, c), f"finalize parts={nparts} c={c}")


@pytest.mark.parametrize("with_dres", [False, True], ids=["nodres", "dres"])
@pytest.mark.parametrize("code", [0, 1], ids=["fp32", "bf16"])
@pytest.mark.parametrize("many", [False, True], ids=["1wg", "3wg"])
@pytest.mark.parametrize("c,nparts", B.BWD_INLINE + B.BWD_FALLTHROUGH, ids=lambda v: str(v))
def test_inline_backward_from_partial_rows(c, nparts, many, code, with_dres):
    """vs_bn_bwd_from_partials: c in 8 / 64 / 512 with at most 64 rows sums inside the apply sweep; 65 rows, or c = 24, take
    bn_bwd_finalize and the plain apply sweep.  dgamma / dbeta: the float64 sum of the fp32 rows, rounded once; dx within its bound;
    dres = g; same bits with and without prefetch"""
    _held(B.inline_backward_figures(c, nparts, many, code, with_dres), f"c={c} parts={nparts}")
