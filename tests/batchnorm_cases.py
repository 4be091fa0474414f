"""What the BatchNorm tests share (tests/test_batchnorm_host.py, tests/test_hip_batchnorm.py, tools/batchnorm_probe.py): seeded inputs,
float64 references, the bounds with their derivations, the launch each case selects, and the figures (measured error over bound) that
a test asserts to be at most 1 and the probe prints.  The kernels are csrc/norm.hip: the two-launch statistics, the plain apply, the
inline apply from fp32 partial rows and from 64-bit fixed-point bins, the two-sweep backward (mask from y or recomputed), the inline
backward, the prefetched form of each, and the evaluation-mode fold.

Every stage is judged from the state the device produced before it (as the AdamW tests judge each step): the apply reference takes
the device's mean / invstd, the backward reference the device's mean / invstd and the y the test hands in, the dx reference the
device's dgamma / dbeta.  The chained cases alone go end to end against float64 F.batch_norm with float64 autograd.

References are torch float64 and run where their tensors live (the host tests on the CPU, the GPU tests on the device: torch's
float64 there, not a kernel of this project).  Inputs are float32 values the device dtype holds exactly, built once per process and
never written to."""
import dataclasses
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from hip_helpers import DEV, option, rounded, tdtype

U = 2.0 ** -24                    # unit roundoff of fp32: one rounding is at most U relative
ITERS_PER_BLOCK, MAX_BLOCKS, KU, KVEC = 4, 1024, 4, 8     # make_rowmap's defaults and the rows per trip (csrc/norm.hip)
EPS_MOM = ((1e-5, 0.1), (1e-3, 0.01))
MARGIN = 1e-3                     # a recomputed (or chained) ReLU mask stays this far from zero, so that no element is ever left out


def gamma_k(k):
    """k roundings in a row: (1 + U)^k - 1 <= k U / (1 - k U)"""
    return k * U / (1.0 - k * U)


def f32(v):
    return float(np.float32(v))


# ---- the launch of a case ------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class RowMap:
    cv: int
    rpb: int
    nblocks: int
    ipb: int

    @property
    def rows_per_block(self):
        return self.ipb * self.rpb

    @property
    def chain(self):
        """L: fp32 adds a thread chains (its rows in order), followed by rpb adds across the row lanes in LDS"""
        return self.ipb


def rowmap(rows, c):
    """make_rowmap of csrc/norm.hip restated: c / 8 channel vectors (at most 256) share a 256-thread block, rpb rows per block iteration,
    a block per 4 iterations until the grid reaches 1024 blocks, then more iterations per block"""
    cv = min(c // KVEC, 256)
    rpb = 256 // cv
    iters = -(-rows // rpb)
    nb = max(1, min(-(-iters // ITERS_PER_BLOCK), MAX_BLOCKS))
    return RowMap(cv, rpb, nb, -(-iters // nb))


def launch(rows, c):
    """what the issue's table names per shape: (nblocks, iterations per block, trips of 4 rows per thread, idle threads per block,
    blocks without a row, rows of the last block that has any, rows live in a thread's last trip of a full block)"""
    m = rowmap(rows, c)
    busy = -(-rows // m.rows_per_block)
    trips = -(-m.ipb // KU)
    return (m.nblocks, m.ipb, trips, 256 - m.cv * m.rpb, m.nblocks - busy, rows - (busy - 1) * m.rows_per_block, m.ipb - KU * (trips - 1))


# (rows, c) -> launch(rows, c), written out by hand from make_rowmap; tests/test_batchnorm_host.py holds the restatement above to it
LAUNCHES = {
    (1, 8): (1, 1, 1, 0, 0, 1, 1),                  # one row: var 0, invstd = 1/sqrt(eps), the unbiased guard; forward only
    (2, 8): (1, 1, 1, 0, 0, 2, 1),                  # the smallest shape for the backward
    (37, 24): (1, 1, 1, 1, 0, 37, 1),               # cv 3, rpb 85, thread 255 idle, one ragged trip
    (70, 48): (1, 2, 1, 4, 0, 70, 2),               # rpb 42, 4 idle threads, rows % rpb = 28
    (27, 512): (2, 4, 1, 0, 0, 11, 4),              # layer4 at a 96-pixel image, batch 3: 2 blocks, the last with 11 rows
    (263, 520): (22, 4, 1, 61, 0, 11, 4),           # cv 65, rpb 3, 61 idle threads
    (700, 304): (30, 4, 1, 28, 0, 4, 4),            # rpb 6, 28 idle threads, last block 4 rows
    (1000, 64): (8, 4, 1, 0, 0, 104, 4),            # the value families' middle shape
    (1025, 2048): (257, 4, 1, 0, 0, 1, 4),          # 257 blocks: the first u = 1 row of the finalise
    (33000, 64): (258, 4, 1, 0, 0, 104, 4),         # 258 blocks at rpb 32
    (4100, 2048): (1024, 5, 2, 0, 204, 5, 1),       # the cap: ipb 5, a second trip with one live row of four, 204 empty blocks
    (524800, 16): (1024, 5, 2, 0, 204, 640, 1),     # fp32 only: the same cap at the 16-channel end, rpb 128
}
SHAPES = [s for s in LAUNCHES if s != (1000, 64)]
FAMILY_SHAPES = [(37, 24), (1000, 64), (4100, 2048)]
FAMILIES = ("plain", "offset", "outlier-K", "constant", "ties")


@dataclasses.dataclass(frozen=True)
class Case:
    """family: plain = 2 randn + 0.5;  offset = mean 300, std 0.05, row 0 drawn like the rest (what the shift K = row 0 exists for;
    bf16 holds 298, 300, 302 there: most of a channel equals K);  outlier-K = plain with row 0 replaced by mean + 50 std (the statistics
    bounds grow with (mean - K)^2);  constant = plain with every eighth channel constant;  ties = plain, and the y handed to the backward
    has more than half exact zeros.
    The branch options each case is run with are the loops of two_sweep_figures: relu and residual of the apply, the mask source
    (none / y / recomputed) and dres of the backward, running statistics null or not, the two (eps, momentum)."""
    rows: int
    c: int
    code: int                    # 0 = fp32, 1 = bf16
    family: str = "plain"

    @property
    def seed(self):
        return 7919 * self.rows + 31 * self.c + 3 * self.code + FAMILIES.index(self.family)

    @property
    def id(self):
        return f"{self.rows}x{self.c}-{'bf16' if self.code else 'fp32'}-{self.family}"

    @property
    def backward(self):
        return self.rows > 1

    @property
    def recompute(self):
        """whether vs_bn_bwd_recompute runs on the case: every family whose inputs a nudge of 0.5 can keep MARGIN away from a zero
        pre-activation - not the offset family, where bf16 holds three values and 0.5 is no step of it"""
        return self.rows > 1 and self.family != "offset"


SHAPE_CASES = [Case(r, c, code) for (r, c) in SHAPES for code in (0, 1) if not (code == 1 and (r, c) == (524800, 16))]
FAMILY_CASES = [Case(r, c, code, fam) for fam in FAMILIES for (r, c) in FAMILY_SHAPES for code in (0, 1)
                if not (fam == "plain" and (r, c) != (1000, 64))]      # (plain at the two other shapes is in SHAPE_CASES)
TWO_SWEEP_CASES = SHAPE_CASES + FAMILY_CASES
CHAINED_CASES = [Case(700, 304, 0), Case(700, 304, 1)]


@functools.lru_cache(maxsize=3)
def inputs(case):
    """x, res, dy, y_ties (ties family, else None), gamma, beta, rm0, rv0 on the CPU.  x is nudged so that the pre-activation
    (x - mean) invstd gamma + beta under its own float64 statistics (eps 1e-5) keeps MARGIN from zero - the recomputed mask then
    never depends on a rounding, and no element has to be left out of a comparison."""
    g = torch.Generator().manual_seed(case.seed)
    rows, c, code = case.rows, case.c, case.code
    if case.family == "offset":
        x = torch.randn(rows, c, generator=g) * 0.05 + 300.0
    else:
        x = torch.randn(rows, c, generator=g) * 2 + 0.5
    if case.family == "outlier-K":
        x[0] = x.double().mean(0).float() + 50 * x.double().std(0, unbiased=False).float()
    if case.family == "constant":
        x[:, ::8] = x[0, ::8].clone()
    x = rounded(x, code)
    res = rounded(torch.randn(rows, c, generator=g), code)
    dy = rounded(torch.randn(rows, c, generator=g), code)
    gamma, beta = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g)
    rm0, rv0 = torch.randn(c, generator=g), torch.rand(c, generator=g) + 0.5
    y_ties = None
    if case.family == "ties":
        y_ties = rounded(torch.randn(rows, c, generator=g).clamp_min(0) * (torch.rand(rows, c, generator=g) > 0.3), code)
    if case.recompute:
        movable = torch.ones(rows, c, dtype=torch.bool)      # what a nudge may touch: not the outlying row 0, not a constant channel
        if case.family == "outlier-K":
            movable[0] = False
        if case.family == "constant":      # (there the pre-activation is beta itself)
            movable[:, ::8] = False
            beta[::8] = torch.where(beta[::8].abs() < 2 * MARGIN, beta[::8] + 0.25, beta[::8])
        for _ in range(8):
            near = (preactivation(x, gamma, beta).abs() < 2 * MARGIN) & movable
            if not near.any():
                break
            x = torch.where(near, rounded(x + 0.5, code), x)
    return x, res, dy, y_ties, gamma, beta, rm0, rv0


def ref_stats(x64):
    mean = x64.mean(0)
    return mean, ((x64 - mean) ** 2).mean(0)


def preactivation(x, gamma, beta, eps=1e-5):
    """(x - mean) invstd gamma + beta in float64 under the float64 statistics of x"""
    x64 = x.double()
    mean, var = ref_stats(x64)
    return (x64 - mean) / torch.sqrt(var + f32(eps)) * gamma.double() + beta.double()


# ---- figures: (label, worst measured error / bound) ----------------------------------------------------------------------------
def worst(err, bound):
    """max over the elements of err / bound; an element with bound 0 must have err 0; NaN (an unwritten element) stays NaN"""
    err, bound = torch.broadcast_tensors(err.double(), bound.double())
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf)))
    if torch.isnan(err).any():
        return math.nan
    return r.max().item()


def half_ulp(v, code):
    """half a unit in the last place of |v| as the output type stores it (bf16: 8 significant bits); fp32 stores are counted among the
    roundings of the expression"""
    if code == 0:
        return torch.zeros_like(v)
    e = ((v.abs().float().view(torch.int32) >> 23) & 0xff) - 127          # floor(log2 |v|) of a normal number
    return torch.exp2((e - 8).double())


def ulps(a, b):
    """distance of two fp32 tensors in units of the last place (0 = equal bits, 1 = neighbours)"""
    def ordered(t):
        i = t.contiguous().view(torch.int32).long()
        return torch.where(i < 0, -(i & 0x7fffffff), i)
    if torch.isnan(a).any() or torch.isnan(b).any():
        return math.nan
    return (ordered(a.float()) - ordered(b.float())).abs().max().item()


# Sums (bn_stats_partial, bn_bwd_partial): a thread chains L fp32 adds (its rows in order), the rpb row lanes of a channel meet in LDS
# with rpb more fp32 adds, and everything after that (the partial rows over the blocks, the division) is fp64.  A term carries at most
# 3 roundings of its own ((x - K), its square; g (x - mean) invstd) and the first add of each chain is exact, so a term passes at most
# L + rpb + 2 roundings:  |err| <= gamma_k(L + rpb + 2) sum |term|, plus one fp32 rounding of the published value.
def sum_factor(m):
    return gamma_k(m.chain + m.rpb + 2)


def stats_figures(x, eps, momentum, rm0, rv0, d_mean, d_invstd, d_rm, d_rv, m, prefix="stats"):
    """vs_bn_stats.  The terms are x - K and (x - K)^2 with K = row 0, not x and x^2: with dm = mean - K,
      |dm_dev - dm| <= B sum|x - K| / n =: e_dm,     mean = dm + K in fp64, rounded once: e_mean = e_dm + U |mean|
      var_dev = q / n - dm_dev^2:   e_var = B sum (x - K)^2 / n + 2 |dm| e_dm + e_dm^2,  and sum (x - K)^2 / n = var + (mean - K)^2 -
      the variance bound carries (mean - K)^2: it is B var when row 0 sits at the mean and grows 2500-fold when row 0 is 50 std out.
      invstd = (var + eps)^-1/2 has slope -1/2 (var + eps)^-3/2, largest at the low end var - e_var (not below 0: the kernel clamps):
      e_invstd = 1/2 (max(var - e_var, 0) + eps)^-3/2 e_var + U invstd.
      running_mean = (1 - mom) rm + mom mean (fp64 from the unrounded mean, one rounding): mom e_dm + U |.|;  running_var likewise with
      the unbiased variance var n / (n - 1), n > 1 (n = 1: var itself)."""
    n = x.shape[0]
    x64 = x.double()
    K = x64[0]
    mean, var = ref_stats(x64)
    B = sum_factor(m)
    dm = mean - K
    e_dm = B * (x64 - K).abs().sum(0) / n
    e_var = B * (var + dm * dm) + 2 * dm.abs() * e_dm + e_dm * e_dm
    eps64, mom = f32(eps), f32(momentum)
    invstd = 1 / torch.sqrt(var + eps64)
    e_is = 0.5 * ((var - e_var).clamp_min(0) + eps64) ** -1.5 * e_var + U * invstd
    out = [(f"{prefix} mean", worst((d_mean.double() - mean).abs(), e_dm + U * mean.abs())),
           (f"{prefix} invstd", worst((d_invstd.double() - invstd).abs(), e_is))]
    if d_rm is not None:
        unb = n / (n - 1) if n > 1 else 1.0
        rm = (1 - mom) * rm0.double() + mom * mean
        rv = (1 - mom) * rv0.double() + mom * var * unb
        out += [(f"{prefix} running_mean", worst((d_rm.double() - rm).abs(), mom * e_dm + U * rm.abs())),
                (f"{prefix} running_var", worst((d_rv.double() - rv).abs(), mom * unb * e_var + U * rv.abs()))]
    return out


APPLY_ROUNDINGS = 5


def apply_reference(x, res, relu, gamma, beta, mean, invstd, code, carried=0.0):
    """y = relu((x - mean) invstd gamma + beta + res) from the given fp32 mean / invstd, and its bound.  The kernel writes
    v = (x - mu) * a + b with a = invstd * gamma, then v += res: roundings of x - mu, a, the product, + b, + res = 5, each relative to a
    partial result no larger than M = |p| + |beta| + |res| (p the exact product), so |err| <= gamma_k(5) M (a contraction into an fma
    only removes one); relu does not increase a difference.  bf16: plus half a unit in the last place of the stored value.
    carried: what the chained cases add for the errors of the stages before."""
    p = (x.double() - mean.double()) * invstd.double() * gamma.double()
    pre = p + beta.double()
    M = p.abs() + beta.double().abs()
    if res is not None:
        pre, M = pre + res.double(), M + res.double().abs()
    ref = pre.clamp_min(0) if relu else pre
    e32 = gamma_k(APPLY_ROUNDINGS) * M + carried
    return ref, e32 + half_ulp(ref.abs() + e32, code)


def apply_figures(label, x, res, relu, gamma, beta, mean, invstd, d_y, code):
    ref, bound = apply_reference(x, res, relu, gamma, beta, mean, invstd, code)
    return [(label, worst((d_y.double() - ref).abs(), bound))]


DX_ROUNDINGS = 8


def masked_gradient(x, dy, y, mode, gamma, beta, mean, invstd):
    """g = dy under the mask: none, y > 0 (strict) of the y handed in, or recomputed as (x - mean) invstd gamma + beta > 0"""
    if mode == "none":
        return dy.double()
    if mode == "y":
        return dy.double() * (y > 0)
    return dy.double() * (((x.double() - mean.double()) * invstd.double() * gamma.double() + beta.double()) > 0)


def bwd_sums_figures(label, g, x, mean, invstd, d_dgamma, d_dbeta, m):
    """dbeta = sum g, dgamma = sum g xhat with xhat = (x - mean) invstd from the device's fp32 mean / invstd: the sum bound above on the
    terms g and g xhat, plus the one rounding of the published fp32 value.  No absolute slack for either dtype."""
    xhat = (x.double() - mean.double()) * invstd.double()
    B = sum_factor(m)
    dbeta, dgamma = g.sum(0), (g * xhat).sum(0)
    return [(f"{label} dbeta", worst((d_dbeta.double() - dbeta).abs(), B * g.abs().sum(0) + U * dbeta.abs())),
            (f"{label} dgamma", worst((d_dgamma.double() - dgamma).abs(), B * (g * xhat).abs().sum(0) + U * dgamma.abs()))]


def dx_reference(g, x, mean, invstd, gamma, dgamma, dbeta, n, code, carried=0.0):
    """dx = gamma invstd (g - dbeta / n - xhat dgamma / n) from the given fp32 dgamma / dbeta, and its bound.  The kernel writes
    gi * (g - db - (x - mu) * is * dg), gi = gamma * invstd, db = dbeta * inv_m, dg = dgamma * inv_m, inv_m = 1.f / n.  Roundings on the
    way of the term g: the two subtractions, gi, the last product = 4; of db: inv_m, its product, and those 4 = 6; of the xhat term:
    x - mu, * is, inv_m, dg, * dg, the second subtraction, gi, the last product = 8.  So |err| <= gamma_k(8) |gamma invstd| (|g| + |db| +
    |xhat dg|); bf16: plus half a unit in the last place of the stored value."""
    xhat = (x.double() - mean.double()) * invstd.double()
    gi = gamma.double() * invstd.double()
    db, dg = dbeta.double() / n, dgamma.double() / n
    ref = gi * (g - db - xhat * dg)
    e32 = gamma_k(DX_ROUNDINGS) * gi.abs() * (g.abs() + db.abs() + (xhat * dg).abs()) + carried
    return ref, e32 + half_ulp(ref.abs() + e32, code)


def dx_figures(label, g, x, mean, invstd, gamma, dgamma, dbeta, d_dx, d_dres, code):
    ref, bound = dx_reference(g, x, mean, invstd, gamma, dgamma, dbeta, x.shape[0], code)
    out = [(f"{label} dx", worst((d_dx.double() - ref).abs(), bound))]
    if d_dres is not None:      # dres = g: a copy of representable values, every bit
        out.append((f"{label} dres", worst((d_dres.double() - g).abs(), torch.zeros((), dtype=torch.float64, device=g.device))))
    return out


def fold_figures(gamma, beta, rm, rv, eps, d_scale, d_shift):
    """vs_bn_fold: s = gamma / sqrtf(rv + eps), shift = beta - rm * s (HIP's fp32 division and square root round correctly).  The sum
    rv + eps is rounded once and the root halves that, then the root and the quotient round: |err s| <= gamma_k(3) |s|.
    shift: |rm| err s, plus the roundings of the product and of the difference, each at most U (|beta| + |rm s|)."""
    s = gamma.double() / torch.sqrt(rv.double() + f32(eps))
    e_s = gamma_k(3) * s.abs()
    shift = beta.double() - rm.double() * s
    return [("fold scale", worst((d_scale.double() - s).abs(), e_s)),
            ("fold shift", worst((d_shift.double() - shift).abs(), rm.double().abs() * e_s + 2 * U * (beta.double().abs() + (rm.double() * s).abs())))]


# ---- stand-in for the device on the CPU (host tests): the same stages in float32 torch ---------------------------------------------
def float32_stages(case, eps=1e-5, momentum=0.1, shifted=False):
    """mean, invstd, running statistics of x in float32 torch; shifted = the float32 NumPy restatement of bn_stats_partial's sums
    (terms x - K, their squares) that stands in where float32 torch, which does not shift, cannot meet a bound on terms of x - K"""
    x, res, dy, y_ties, gamma, beta, rm0, rv0 = inputs(case)
    n = x.shape[0]
    if shifted:
        xs = x.numpy()
        m = rowmap(n, case.c)
        d = np.zeros((m.nblocks * m.rows_per_block, case.c), np.float32)
        d[:n] = xs - xs[0]
        d = d.reshape(m.nblocks, m.ipb, m.rpb, case.c)      # [block][iteration][row lane]: fp32 over a thread's rows, then over the lanes; fp64 after
        s32 = lambda t: t.sum(1, dtype=np.float32).sum(1, dtype=np.float32).astype(np.float64).sum(0)
        dm = s32(d) / n
        var = torch.tensor(np.maximum(s32(d * d) / n - dm * dm, 0.0))
        mean64 = torch.tensor(dm + xs[0].astype(np.float64))
    else:
        mean64, var = x.mean(0).double(), x.var(0, unbiased=False).double()
    mean, invstd = mean64.float(), (1 / torch.sqrt(var + f32(eps))).float()
    mom, unb = f32(momentum), (n / (n - 1) if n > 1 else 1.0)
    rm = ((1 - mom) * rm0.double() + mom * mean64).float()
    rv = ((1 - mom) * rv0.double() + mom * var * unb).float()
    return mean, invstd, rm, rv


def float32_apply(x, res, relu, gamma, beta, mean, invstd, code):
    v = (x - mean) * (invstd * gamma) + beta
    if res is not None:
        v = v + res
    return rounded(v.clamp_min(0) if relu else v, code)


def float32_bwd(g, x, mean, invstd, gamma, code):
    g = g.float()
    xhat = (x - mean) * invstd
    dbeta, dgamma = g.sum(0), (g * xhat).sum(0)
    inv_m = np.float32(1.0) / np.float32(x.shape[0])
    dx = gamma * invstd * (g - dbeta * inv_m - xhat * (dgamma * inv_m))
    return rounded(dx, code), dgamma, dbeta


# ---- device runs ---------------------------------------------------------------------------------------------------------------
NAN = float("nan")


def _L():
    from volume_segmantics_amd import _lib
    return _lib


def _nan(shape, dtype=torch.float32):
    return torch.full(shape, NAN, device=DEV, dtype=dtype)


def _workspace(L, rows, c):
    wsb = L.lib.vs_bn_workspace(rows, c)
    return torch.empty(wsb, dtype=torch.uint8, device=DEV), wsb


def two_sweep_figures(case):
    """vs_bn_stats, vs_bn_apply, vs_bn_bwd and vs_bn_bwd_recompute on one case, every output NaN-filled beforehand:
    statistics with running statistics null and not null under both (eps, momentum); the apply with relu 0 / 1 and residual absent /
    present; the backward with no mask, the mask from y (the reference y of the apply with residual, rounded to the dtype; the ties
    family hands in its own y) and the recomputed mask (every family but offset, see Case.recompute), dres absent / present."""
    L = _L()
    x, res, dy, y_ties, gamma, beta, rm0, rv0 = (None if t is None else t.to(DEV) for t in inputs(case))
    rows, c, code = case.rows, case.c, case.code
    dt, m = tdtype(code), rowmap(rows, c)
    xd, resd, dyd = x.to(dt), res.to(dt), dy.to(dt)
    ws, wsb = _workspace(L, rows, c)
    out = []
    for eps, mom in reversed(EPS_MOM):
        for running in (False, True):
            mean, invstd = _nan((c,)), _nan((c,))
            rm, rv = (rm0.clone(), rv0.clone()) if running else (None, None)
            L.check(L.lib.vs_bn_stats(code, L.ptr(xd), rows, c, eps, mom, L.ptr(mean), L.ptr(invstd), L.ptr(rm), L.ptr(rv), L.ptr(ws), wsb, None))
            out += stats_figures(x, eps, mom, rm0, rv0, mean, invstd, rm, rv, m, f"stats eps={eps:g} run={int(running)}")
            if case.family == "constant":       # exact variance 0: invstd is float32(1 / sqrt(eps)) to the bit
                want = np.float32(1.0 / math.sqrt(f32(eps)))
                out.append((f"constant channels eps={eps:g} exact invstd", 0.0 if bool((invstd[::8] == float(want)).all()) else math.inf))
    for relu in (0, 1):         # (mean, invstd: those of the last statistics launch, eps 1e-5; the backward below takes them too)
        for r in (None, res):
            y = _nan((rows, c), dt)
            L.check(L.lib.vs_bn_apply(code, L.ptr(xd), L.ptr(mean), L.ptr(invstd), L.ptr(gamma), L.ptr(beta), None if r is None else L.ptr(resd), relu,
                                      L.ptr(y), rows, c, None))
            out += apply_figures(f"apply relu={relu} res={int(r is not None)}", x, r, relu, gamma, beta, mean, invstd, y, code)
    if not case.backward:
        return out
    if y_ties is not None:
        y_in = y_ties
    else:
        y_in = rounded(apply_reference(x, res, 1, gamma, beta, mean, invstd, code)[0].float(), code)
    yd = y_in.to(dt)
    modes = ("none", "y", "recompute") if case.recompute else ("none", "y")
    if case.recompute:      # the margin holds under the device's statistics too
        pre = (x.double() - mean.double()) * invstd.double() * gamma.double() + beta.double()
        out.append(("recomputed mask margin", 0.0 if pre.abs().min().item() >= MARGIN else math.inf))
    for mode in modes:
        g = masked_gradient(x, dy, y_in, mode, gamma, beta, mean, invstd)
        for with_dres in (False, True):
            dx, dres = _nan((rows, c), dt), (_nan((rows, c), dt) if with_dres else None)
            dgamma, dbeta = _nan((c,)), _nan((c,))
            if mode == "recompute":
                L.check(L.lib.vs_bn_bwd_recompute(code, L.ptr(dyd), None, L.ptr(xd), L.ptr(mean), L.ptr(invstd), L.ptr(gamma), L.ptr(beta), 1,
                                                  L.ptr(dx), L.ptr(dres), L.ptr(dgamma), L.ptr(dbeta), rows, c, L.ptr(ws), wsb, None))
            else:
                relu = int(mode == "y")
                L.check(L.lib.vs_bn_bwd(code, L.ptr(dyd), L.ptr(yd) if relu else None, L.ptr(xd), L.ptr(mean), L.ptr(invstd), L.ptr(gamma), relu,
                                        L.ptr(dx), L.ptr(dres), L.ptr(dgamma), L.ptr(dbeta), rows, c, L.ptr(ws), wsb, None))
            label = f"bwd mask={mode} dres={int(with_dres)}"
            out += bwd_sums_figures(label, g, x, mean, invstd, dgamma, dbeta, m)
            out += dx_figures(label, g, x, mean, invstd, gamma, dgamma, dbeta, dx, dres, code)
    torch.cuda.synchronize()
    return out


# ---- chained: statistics -> apply -> backward against float64 F.batch_norm with float64 autograd -----------------------------------
@functools.lru_cache(maxsize=2)
def chained_inputs(case):
    """as inputs(case), with the residual nudged so that bn(x) + res keeps MARGIN from zero: the mask y > 0 of the device's y is then
    the mask of the reference (the device's pre-activation is within 1e-5 of it), and every element is compared"""
    x, res, dy, _, gamma, beta, rm0, rv0 = inputs(case)
    near = (preactivation(x, gamma, beta) + res.double()).abs() < 2 * MARGIN
    res = torch.where(near, rounded(res + 0.25, case.code), res)
    assert (preactivation(x, gamma, beta) + res.double()).abs().min() >= MARGIN
    return x, res, dy, gamma, beta, rm0, rv0


def chained_reference(x, res, dy, gamma, beta, rm0, rv0, eps=1e-5, momentum=0.1):
    """y = relu(batch_norm(x) + res) and the gradients of sum(y dy), float64 throughout ([rows][c] viewed as N = rows, C = c)"""
    xr, rr = x.double().requires_grad_(), res.double().requires_grad_()
    gr, br = gamma.double().requires_grad_(), beta.double().requires_grad_()
    rm, rv = rm0.double().clone(), rv0.double().clone()
    y = (F.batch_norm(xr, rm, rv, gr, br, training=True, momentum=f32(momentum), eps=f32(eps)) + rr).relu()
    y.backward(dy.double())
    return y.detach(), xr.grad, rr.grad, gr.grad, br.grad, rm, rv


def chained_figures(case, got):
    """got = (mean, invstd, rm, rv, y, dx, dres, dgamma, dbeta) of the three stages run one after the other.  The stage bounds above,
    with the errors of the earlier stages carried forward to first order (products of two errors are U^2 and left out):
      y:       the apply bound + |invstd gamma| e_mean + |x - mean| |gamma| e_invstd
      xhat:    e_xhat = invstd e_mean + |x - mean| e_invstd
      dbeta:   the sum bound;    dgamma: the sum bound + sum |g| e_xhat
      dx:      the dx bound + |gamma| e_invstd |g - dbeta/n - xhat dgamma/n| + |gamma invstd| (e_dbeta / n + e_xhat |dgamma| / n + |xhat| e_dgamma / n)"""
    x, res, dy, gamma, beta, rm0, rv0 = (t.to(got[0].device) for t in chained_inputs(case))
    n, code, m = case.rows, case.code, rowmap(case.rows, case.c)
    ry, rdx, rdres, rdgamma, rdbeta, rrm, rrv = chained_reference(x, res, dy, gamma, beta, rm0, rv0)
    d_mean, d_invstd, d_rm, d_rv, d_y, d_dx, d_dres, d_dgamma, d_dbeta = got
    out = stats_figures(x, 1e-5, 0.1, rm0, rv0, d_mean, d_invstd, d_rm, d_rv, m, "chained")
    x64, g64, ga = x.double(), gamma.double(), gamma.double().abs()
    K = x64[0]
    mean, var = ref_stats(x64)
    B = sum_factor(m)
    dm = mean - K
    e_dm = B * (x64 - K).abs().sum(0) / n
    e_mean = e_dm + U * mean.abs()
    e_var = B * (var + dm * dm) + 2 * dm.abs() * e_dm + e_dm * e_dm
    invstd = 1 / torch.sqrt(var + f32(1e-5))
    e_is = 0.5 * ((var - e_var).clamp_min(0) + f32(1e-5)) ** -1.5 * e_var + U * invstd
    _, b_y = apply_reference(x, res, 1, gamma, beta, mean, invstd, code, invstd * ga * e_mean + (x64 - mean).abs() * ga * e_is)
    out.append(("chained y", worst((d_y.double() - ry).abs(), b_y)))
    g = dy.double() * (ry > 0)
    xhat = (x64 - mean) * invstd
    e_xhat = invstd * e_mean + (x64 - mean).abs() * e_is
    e_db = B * g.abs().sum(0) + U * rdbeta.abs()
    e_dg = B * (g * xhat).abs().sum(0) + U * rdgamma.abs() + (g.abs() * e_xhat).sum(0)
    out += [("chained dbeta", worst((d_dbeta.double() - rdbeta).abs(), e_db)), ("chained dgamma", worst((d_dgamma.double() - rdgamma).abs(), e_dg)),
            ("chained dres", worst((d_dres.double() - rdres).abs(), torch.zeros((), dtype=torch.float64, device=x.device)))]
    inner = (g - rdbeta / n - xhat * rdgamma / n).abs()
    carried = ga * e_is * inner + ga * invstd * (e_db / n + e_xhat * rdgamma.abs() / n + xhat.abs() * e_dg / n)
    _, b_dx = dx_reference(g, x, mean, invstd, gamma, rdgamma, rdbeta, n, code, carried)
    out.append(("chained dx", worst((d_dx.double() - rdx).abs(), b_dx)))
    return out


def chained_device(case):
    L = _L()
    x, res, dy, gamma, beta, rm0, rv0 = (t.to(DEV) for t in chained_inputs(case))
    rows, c, code = case.rows, case.c, case.code
    dt = tdtype(code)
    xd, resd, dyd = x.to(dt), res.to(dt), dy.to(dt)
    ws, wsb = _workspace(L, rows, c)
    mean, invstd, rm, rv = _nan((c,)), _nan((c,)), rm0.clone(), rv0.clone()
    y, dx, dres, dgamma, dbeta = _nan((rows, c), dt), _nan((rows, c), dt), _nan((rows, c), dt), _nan((c,)), _nan((c,))
    L.check(L.lib.vs_bn_stats(code, L.ptr(xd), rows, c, 1e-5, 0.1, L.ptr(mean), L.ptr(invstd), L.ptr(rm), L.ptr(rv), L.ptr(ws), wsb, None))
    L.check(L.lib.vs_bn_apply(code, L.ptr(xd), L.ptr(mean), L.ptr(invstd), L.ptr(gamma), L.ptr(beta), L.ptr(resd), 1, L.ptr(y), rows, c, None))
    L.check(L.lib.vs_bn_bwd(code, L.ptr(dyd), L.ptr(y), L.ptr(xd), L.ptr(mean), L.ptr(invstd), L.ptr(gamma), 1, L.ptr(dx), L.ptr(dres),
                            L.ptr(dgamma), L.ptr(dbeta), rows, c, L.ptr(ws), wsb, None))
    torch.cuda.synchronize()
    return mean, invstd, rm, rv, y, dx, dres, dgamma, dbeta


# ---- vs_bn_fold ----------------------------------------------------------------------------------------------------------------
FOLD_C = (8, 96, 2048)


@functools.lru_cache(maxsize=None)
def fold_inputs(c):
    """running_var down to exactly 0 (every fifth channel), tiny and ordinary values between"""
    g = torch.Generator().manual_seed(400 + c)
    gamma, beta, rm = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g), torch.randn(c, generator=g) * 3
    rv = torch.rand(c, generator=g) * 10.0 ** torch.randint(-8, 1, (c,), generator=g).float()
    rv[::5] = 0.0
    return gamma, beta, rm, rv


def fold_device(c, eps):
    L = _L()
    gamma, beta, rm, rv = (t.to(DEV) for t in fold_inputs(c))
    sc, sh = _nan((c,)), _nan((c,))
    L.check(L.lib.vs_bn_fold(L.ptr(gamma), L.ptr(beta), L.ptr(rm), L.ptr(rv), eps, L.ptr(sc), L.ptr(sh), c, None))
    torch.cuda.synchronize()
    return fold_figures(gamma, beta, rm, rv, eps, sc, sh)


# ---- the inline sweeps through the test seams -----------------------------------------------------------------------------------
# Sums the caller wrote: the float64 per-channel sums of x, split over nparts rows of unequal share, every fifth share negative, each
# rounded to fp32.  The statistics are DEFINED from those fp32 values - mean = sum s / n, var = sum q / n - mean^2 in float64 - and
# the kernels form them in fp64 too, in another order (row groups, butterflies) and with fused multiply-adds where the compiler
# contracts: the two doubles agree to some 1e-13 relative, so the published fp32 values are the rounding of the reference or, where
# the double falls that close to the middle between two fp32 numbers, its neighbour: at most 1 unit in the last place, for mean,
# invstd and the running statistics alike.  (The same holds for the bins, whose integer sums are exact.)
INLINE_NPARTS = (1, 3, 64, 257, 1100)
INLINE_C = (8, 64, 512, 24, 1024)          # all-threads branch with 64, 8 and 1 row groups; 24 and 1024: the per-channel fallback
BINS_NB = (1, 8, 64)
BINS_C = (8, 128, 136, 512, 2048)          # 2 c <= 256: row groups in LDS;  2 c > 256: a column per thread
FINALIZE_NPARTS = (1, 257, 1100)
BWD_INLINE = [(c, nparts) for c in (8, 64, 512) for nparts in (1, 3, 64)]                # summed inside the apply sweep
BWD_FALLTHROUGH = [(8, 65), (64, 65), (512, 65), (24, 3), (24, 65)]                      # bn_bwd_finalize + the plain apply sweep


def inline_rows(c, many):
    """rows of one workgroup (3 block iterations, the last ragged) or of three (10 iterations, 4 per workgroup, ragged)"""
    rpb = rowmap(1, c).rpb
    return 9 * rpb + 1 if many else 3 * rpb - 1


@dataclasses.dataclass(frozen=True)
class InlineCase:
    c: int
    nparts: int
    many: bool
    code: int
    stat_rows_factor: int = 1

    @property
    def rows(self):
        return inline_rows(self.c, self.many)

    @property
    def id(self):
        return f"c{self.c}-parts{self.nparts}-{'3wg' if self.many else '1wg'}-{'bf16' if self.code else 'fp32'}" + ("-statrows2x" if self.stat_rows_factor > 1 else "")


PARTIALS_CASES = [InlineCase(c, p, many, code) for c in INLINE_C for p in INLINE_NPARTS for many in (False, True) for code in (0, 1)]
BINS_CASES = ([InlineCase(c, nb, many, code) for c in BINS_C for nb in BINS_NB for many in (False, True) for code in (0, 1)] +
              [InlineCase(128, 8, True, 1, 2), InlineCase(512, 8, True, 0, 2)])


@functools.lru_cache(maxsize=4)
def inline_inputs(c, rows, code):
    """x with channel means of both signs (every third channel negative), res, gamma, beta, rm0, rv0; g (a masked gradient: a third of it
    exact zeros) and fp32 mean / invstd for the backward"""
    gen = torch.Generator().manual_seed(90001 + 17 * c + rows + code)
    off = torch.where(torch.arange(c) % 3 == 0, -1.5, 0.5)
    x = rounded(torch.randn(rows, c, generator=gen) * 2 + off, code)
    res = rounded(torch.randn(rows, c, generator=gen), code)
    gamma, beta = torch.rand(c, generator=gen) + 0.5, torch.randn(c, generator=gen)
    rm0, rv0 = torch.randn(c, generator=gen), torch.rand(c, generator=gen) + 0.5
    g = rounded(torch.randn(rows, c, generator=gen) * (torch.rand(rows, c, generator=gen) > 0.33), code)
    mean, var = ref_stats(x.double())
    return x, res, gamma, beta, rm0, rv0, g, mean.float(), (1 / torch.sqrt(var + f32(1e-5))).float()


def shares(nparts, seed):
    """unequal shares that sum to 1, every fifth negative"""
    w = np.random.default_rng(seed).uniform(0.2, 1.8, nparts)
    w[4::5] *= -0.5
    return w / w.sum()


def split_rows(s, q, nparts, seed):
    """[nparts][2][c] fp32: the float64 sums s, q spread over the rows"""
    w = torch.tensor(shares(nparts, seed))
    return torch.stack([w[:, None] * s[None, :], w[:, None] * q[None, :]], 1).float().contiguous()


def split_bins(s, q, nb, seed):
    """[nb][2][c] int64: round(s 2^24), round(q 2^16) spread over the rows with signed entries (the last row takes the remainder)"""
    L = _L()
    tot = torch.stack([torch.round(s * L.lib.vs_stat_scale(0)), torch.round(q * L.lib.vs_stat_scale(1))]).long()      # [2][c]
    w = torch.tensor(shares(nb, seed))
    rows = torch.round(w[:, None, None] * tot[None].double()).long()
    rows[-1] += tot - rows.sum(0)
    assert torch.equal(rows.sum(0), tot)
    return rows.contiguous(), tot


def defined_stats(s_tot, q_tot, n, eps, momentum, rm0, rv0):
    """mean, invstd, running statistics in float64 from the float64 totals of the rows handed in"""
    mean = s_tot / n
    var = (q_tot / n - mean * mean).clamp_min(0)
    mom, unb = f32(momentum), (n / (n - 1) if n > 1 else 1.0)
    return (mean, 1 / torch.sqrt(var + f32(eps)), (1 - mom) * rm0.double() + mom * mean, (1 - mom) * rv0.double() + mom * var * unb)


def published_figures(label, want, got):
    return [(f"{label} {name} ulps", float(ulps(g, w.float()))) for name, w, g in zip(("mean", "invstd", "running_mean", "running_var"), want, got)
            if g is not None]


def inline_forward_figures(case, source, eps=1e-5, momentum=0.1):
    """vs_bn_apply_from_partials / vs_bn_apply_from_bins under bn_prefetch 0 and 1: the published statistics within 1 ulp of their
    definition (the running statistics one momentum step from rm0 / rv0: workgroup 0 alone publishes), y (residual, relu) within the
    apply bound from the published mean / invstd, and equal bits between the two forms"""
    L = _L()
    c, rows, code, n_stat = case.c, case.rows, case.code, case.rows * case.stat_rows_factor
    x, res, gamma, beta, rm0, rv0 = (t.to(DEV) for t in inline_inputs(c, rows, code)[:6])
    s, q = x.double().sum(0), (x.double() ** 2).sum(0)
    if source == "bins":
        rowsd, tot = split_bins(s.cpu(), q.cpu(), case.nparts, case.nparts + c)
        s_tot, q_tot = tot[0].double() / L.lib.vs_stat_scale(0), tot[1].double() / L.lib.vs_stat_scale(1)
    else:
        rowsd = split_rows(s.cpu(), q.cpu(), case.nparts, case.nparts + c)
        s_tot, q_tot = rowsd[:, 0].double().sum(0), rowsd[:, 1].double().sum(0)
    rowsd = rowsd.to(DEV)
    want = defined_stats(s_tot.to(DEV), q_tot.to(DEV), n_stat, eps, momentum, rm0, rv0)
    dt = tdtype(code)
    xd, resd = x.to(dt), res.to(dt)
    out, runs = [], []
    for pf in (0, 1):
        with option(bn_prefetch=pf):
            mean, invstd, rm, rv, y = _nan((c,)), _nan((c,)), rm0.clone(), rv0.clone(), _nan((rows, c), dt)
            if source == "bins":
                L.check(L.lib.vs_bn_apply_from_bins(code, L.ptr(xd), L.ptr(rowsd), case.nparts, eps, momentum, L.ptr(mean), L.ptr(invstd), L.ptr(rm),
                                                    L.ptr(rv), L.ptr(gamma), L.ptr(beta), L.ptr(resd), 1, L.ptr(y), rows, c,
                                                    n_stat if case.stat_rows_factor > 1 else 0, None))
            else:
                L.check(L.lib.vs_bn_apply_from_partials(code, L.ptr(xd), L.ptr(rowsd), case.nparts, eps, momentum, L.ptr(mean), L.ptr(invstd),
                                                        L.ptr(rm), L.ptr(rv), L.ptr(gamma), L.ptr(beta), L.ptr(resd), 1, L.ptr(y), rows, c, None))
            torch.cuda.synchronize()
        out += published_figures(f"pf={pf}", want, (mean, invstd, rm, rv))
        out += apply_figures(f"pf={pf} y", x, res, 1, gamma, beta, mean, invstd, y, code)
        runs.append((mean, invstd, rm, rv, y))
    same = all(torch.equal(a, b) for a, b in zip(*runs))
    out.append(("prefetch forms differ", 0.0 if same else math.inf))
    return out


def inline_null_running_figures(c, source):
    """running statistics absent, relu 0, no residual: the other side of those branches of the inline apply (fp32, three workgroups)"""
    L = _L()
    case = InlineCase(c, 3, True, 0)
    rows = case.rows
    x, _, gamma, beta, rm0, rv0 = (t.to(DEV) for t in inline_inputs(c, rows, 0)[:6])
    s, q = x.double().sum(0).cpu(), (x.double() ** 2).sum(0).cpu()
    mean, invstd, y = _nan((c,)), _nan((c,)), _nan((rows, c))
    if source == "bins":
        rowsd, tot = split_bins(s, q, 8, 5)
        s_tot, q_tot = tot[0].double() / L.lib.vs_stat_scale(0), tot[1].double() / L.lib.vs_stat_scale(1)
        rowsd = rowsd.to(DEV)
        L.check(L.lib.vs_bn_apply_from_bins(0, L.ptr(x), L.ptr(rowsd), 8, 1e-3, 0.01, L.ptr(mean), L.ptr(invstd), None, None, L.ptr(gamma), L.ptr(beta),
                                            None, 0, L.ptr(y), rows, c, 0, None))
    else:
        rowsd = split_rows(s, q, 3, 5)
        s_tot, q_tot = rowsd[:, 0].double().sum(0), rowsd[:, 1].double().sum(0)
        rowsd = rowsd.to(DEV)
        L.check(L.lib.vs_bn_apply_from_partials(0, L.ptr(x), L.ptr(rowsd), 3, 1e-3, 0.01, L.ptr(mean), L.ptr(invstd), None, None, L.ptr(gamma),
                                                L.ptr(beta), None, 0, L.ptr(y), rows, c, None))
    torch.cuda.synchronize()
    want = defined_stats(s_tot.to(DEV), q_tot.to(DEV), rows, 1e-3, 0.01, rm0, rv0)
    return published_figures("no running", want, (mean, invstd, None, None)) + apply_figures("no running y", x, None, 0, gamma, beta, mean, invstd, y, 0)


def finalize_figures(nparts, c, rows=1000, eps=1e-5, momentum=0.1):
    """vs_bn_finalize_partials on nparts rows: 257 reaches the second of the four rows a thread of strided_sum2_f64 loads per trip,
    1100 all four and a second trip"""
    L = _L()
    x, _, _, _, rm0, rv0 = (t.to(DEV) for t in inline_inputs(c, rows, 0)[:6])
    rowsd = split_rows(x.double().sum(0).cpu(), (x.double() ** 2).sum(0).cpu(), nparts, nparts + c).to(DEV)
    want = defined_stats(rowsd[:, 0].double().sum(0), rowsd[:, 1].double().sum(0), rows, eps, momentum, rm0, rv0)
    mean, invstd, rm, rv = _nan((c,)), _nan((c,)), rm0.clone(), rv0.clone()
    L.check(L.lib.vs_bn_finalize_partials(L.ptr(rowsd), nparts, c, rows, eps, momentum, L.ptr(mean), L.ptr(invstd), L.ptr(rm), L.ptr(rv), None))
    torch.cuda.synchronize()
    return published_figures("finalize", want, (mean, invstd, rm, rv))


def inline_backward_figures(c, nparts, many, code, with_dres):
    """vs_bn_bwd_from_partials under bn_prefetch 0 and 1: rows of (sum g, sum g xhat) split as above; dgamma / dbeta are the float64 sum
    of the fp32 rows handed in, rounded once (within 1 ulp, for the reason above); dx within the dx bound from the published sums;
    dres = g to the bit; equal bits between the two forms"""
    L = _L()
    rows = inline_rows(c, many)
    x, _, gamma, _, _, _, g, mean, invstd = (t.to(DEV) for t in inline_inputs(c, rows, code))
    g64 = g.double()
    xhat = (x.double() - mean.double()) * invstd.double()
    rowsd = split_rows(g64.sum(0).cpu(), (g64 * xhat).sum(0).cpu(), nparts, nparts + c).to(DEV)
    want_db, want_dg = rowsd[:, 0].double().sum(0).float(), rowsd[:, 1].double().sum(0).float()
    dt = tdtype(code)
    xd, gd = x.to(dt), g.to(dt)
    out, runs = [], []
    for pf in (0, 1):
        with option(bn_prefetch=pf):
            dx, dres = _nan((rows, c), dt), (_nan((rows, c), dt) if with_dres else None)
            dgamma, dbeta = _nan((c,)), _nan((c,))
            L.check(L.lib.vs_bn_bwd_from_partials(code, L.ptr(gd), L.ptr(xd), L.ptr(mean), L.ptr(invstd), L.ptr(gamma), L.ptr(dx), L.ptr(dres),
                                                  L.ptr(dgamma), L.ptr(dbeta), rows, c, L.ptr(rowsd), nparts, None))
            torch.cuda.synchronize()
        out += [(f"pf={pf} dbeta ulps", float(ulps(dbeta, want_db))), (f"pf={pf} dgamma ulps", float(ulps(dgamma, want_dg)))]
        out += dx_figures(f"pf={pf}", g64, x, mean, invstd, gamma, dgamma, dbeta, dx, dres, code)
        runs.append([t for t in (dx, dres, dgamma, dbeta) if t is not None])
    same = all(torch.equal(a, b) for a, b in zip(*runs))
    out.append(("prefetch forms differ", 0.0 if same else math.inf))
    return out


# ---- the convolution epilogue's statistics at non-zero mean (tests/test_hip_ring_kernels.py, the probe's rho curve) -------------------
# ring::conv_ring_kernel ends in conv_epilogue (csrc/conv_common.h): per output channel and pixel tile, a lane adds its PT fp32
# accumulators (and their squares), 16 lanes meet in a 4-level butterfly, the NW waves' values are added in LDS - no term passes more
# than PT + 4 + NW roundings (one more for a square) - and the tile's two fp32 sums go out as a partial row or, rounded to the
# nearest integer of 2^24 (sum) / 2^16 (sum of squares), into a 64-bit bin by one atomic add each.  The consumers form
# var = q / n - mean^2 in fp64, unshifted.  Against the float64 convolution of the same bf16 operands, with a_i the accumulator of
# the terms taken as the float64 values x_i of the convolution of the same bf16 operands, the bound has the issue's terms and no other:
#   E1   = gamma_k(PT + 4 + NW) sum |x| + tiles 2^-25                    (bins only: half a unit of 2^-24 per atomic add)
#   E2   = gamma_k(PT + 5 + NW) sum x^2 + tiles 2^-17                    (the longest per-tile chain; half a unit of 2^-16 per add)
#   |var - var_ref| <= E2 / n + 2 |mean| E1 / n + (E1 / n)^2             - relative to var about gamma_k(..) (1 + 3 rho^2), rho = |mean| / std
# The fp32 accumulators' own distance from x_i (K = 9 cin products through the matrix unit, whose rounding is not documented) has no
# term: a worst-case one (some 150 roundings of one sign on sum_k |x_k w_k|) is a thousand times the rest and would hold the variance
# to nothing; the bound as it stands allows the accumulators a share of the chain's 11 to 15 roundings, and a device that misses it
# has accumulators worth a finding.  The rounding of the bins themselves is also held on its own, against the partial rows of the same
# launch (ring_nonzero_mean_figures).
RING_TILE = {16: (2, 8), 8: (2, 4)}      # image side -> (PT, NW) of the ring kernel that runs it: 256- and 128-pixel tiles


@functools.lru_cache(maxsize=2)
def ring_inputs(h, w, cin, cout, n=32):
    """|randn| input (a post-ReLU-like positive mean), weights randn / sqrt(K) plus a per-output-channel constant d_k on the centre tap,
    chosen so that rho = |mean| / std of output channel k runs log-spaced from about 0 (d = 0) up: with E x = 0.8, Var x = 0.36,
    rho ~ 1.33 sqrt(cin) t / sqrt(1 + t^2), t = d sqrt(cin).  (The centre tap alone: the other eight see the zero padding, and a constant
    on them makes the border pixels' level differ from the interior's, which caps rho near 6.  A sum of cin such inputs cannot exceed
    rho = 1.33 sqrt(cin), so the top of the range is the smaller of 32 and 0.9 of that: 27 at 512 channels, 19 at 256.)
    Returns x (NCHW), w (OIHW), both bf16-exact, and the float64 reference out [n h w][cout]."""
    g = torch.Generator().manual_seed(53 + h)
    K = 9 * cin
    x = rounded(torch.randn(n, cin, h, w, generator=g).abs(), 1)
    top = min(32.0, 0.9 * 4 / 3 * math.sqrt(cin))
    rho = torch.cat([torch.zeros(1), torch.logspace(-1, math.log10(top), cout - 1)])
    r = (rho / (4 / 3 * math.sqrt(cin))).double()
    d = (r / torch.sqrt(1 - r * r) / math.sqrt(cin)).float()
    wt = torch.randn(cout, cin, 3, 3, generator=g) / K ** 0.5
    wt[:, :, 1, 1] += d.view(-1, 1)
    wt = rounded(wt, 1)
    cols = F.unfold(x.double(), 3, padding=1).transpose(1, 2).reshape(n * h * w, K)        # [pixel][cin 3 3]
    wm = wt.double().reshape(cout, K).t()
    return x, wt, cols @ wm


def ring_variance_figures(h, cin, cout, s1, s2, tiles, bins, n=32):
    """figures of the per-channel variance from the epilogue's sums s1, s2 (float64 totals, CPU), and the rho curve: per channel
    (rho, relative error of var, relative error of invstd at eps 1e-5, bound of var relative)"""
    _, _, ref = ring_inputs(h, h, cin, cout, n)
    rows = ref.shape[0]
    pt, nw = RING_TILE[h]
    E1 = gamma_k(pt + 4 + nw) * ref.abs().sum(0) + (tiles * 2.0 ** -25 if bins else 0.0)
    E2 = gamma_k(pt + 5 + nw) * (ref ** 2).sum(0) + (tiles * 2.0 ** -17 if bins else 0.0)
    mean_ref, var_ref = ref_stats(ref)
    e_mean = E1 / rows
    e_var = E2 / rows + 2 * mean_ref.abs() * e_mean + e_mean ** 2
    mean, var = s1 / rows, s2 / rows - (s1 / rows) ** 2
    rho = mean_ref.abs() / var_ref.sqrt()
    is_ref, is_dev = 1 / torch.sqrt(var_ref + f32(1e-5)), 1 / torch.sqrt(var.clamp_min(0) + f32(1e-5))
    curve = torch.stack([rho, (var - var_ref).abs() / var_ref, (is_dev - is_ref).abs() / is_ref, e_var / var_ref], 1)
    figures = [("epilogue mean", worst((mean - mean_ref).abs(), e_mean)), ("epilogue var", worst((var - var_ref).abs(), e_var))]
    return figures, curve, (e_mean, e_var)


def ring_apply_figures(h, cin, cout, conv_out, bins, nb, tiles, n=32):
    """the bins of that launch fed to vs_bn_apply_from_bins with the launch's bf16 output: y against the float64 BatchNorm (eps 1e-5, no
    relu) of the float64 convolution.  Bound: the stored activation differs from the exact one by half a bf16 unit in the last place,
    the mean by e_mean, invstd by what e_var implies (its slope at the low end of the variance), on top of the apply bound."""
    L = _L()
    _, _, ref = ring_inputs(h, h, cin, cout, n)
    rows = ref.shape[0]
    g = torch.Generator().manual_seed(77)
    gamma, beta = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g)
    tot = bins.sum(0).cpu().double()
    _, _, (e_mean, e_var) = ring_variance_figures(h, cin, cout, tot[0] / L.lib.vs_stat_scale(0), tot[1] / L.lib.vs_stat_scale(1), tiles, True, n)
    mean, invstd, y = _nan((cout,)), _nan((cout,)), _nan((rows, cout), torch.bfloat16)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    L.check(L.lib.vs_bn_apply_from_bins(1, L.ptr(conv_out), L.ptr(bins), nb, 1e-5, 0.1, L.ptr(mean), L.ptr(invstd), None, None, L.ptr(gd), L.ptr(bd), None, 0,
                                        L.ptr(y), rows, cout, 0, None))
    torch.cuda.synchronize()
    mean_ref, var_ref = ref_stats(ref)
    eps = f32(1e-5)
    is_ref = 1 / torch.sqrt(var_ref + eps)
    e_is = 0.5 * ((var_ref - e_var).clamp_min(0) + eps) ** -1.5 * e_var + U * is_ref
    e_x = half_ulp(ref.abs(), 1)
    carried = gamma.double() * (is_ref * (e_x + e_mean + U * mean_ref.abs()) + (ref - mean_ref).abs() * e_is)
    want, bound = apply_reference(ref, None, 0, gamma, beta, mean_ref, is_ref, 1, carried)
    return [("epilogue invstd", worst((invstd.cpu().double() - is_ref).abs(), e_is)), ("y from the bins", worst((y.cpu().double() - want).abs(), bound))]


def ring_nonzero_mean_figures(h, cin, cout, stats, variant, n=32):
    """one vs_conv2d_train launch of the 3 x 3 layer on ring_inputs with its statistics epilogue (stats: "bins" - 16 rows of them - or
    "rows"), which must select kernel `variant`: the stored output against the reference at the tolerance of the zero-mean test, the
    figures of the sums, and for the bins those of vs_bn_apply_from_bins.  Returns (figures, rho curve)."""
    import ctypes
    from hip_helpers import conv_desc, to_nhwc, tol, w_krsc
    L = _L()
    x, wt, ref = ring_inputs(h, h, cin, cout, n)
    d = conv_desc(L, 1, n, h, h, cin, cout, 3, 1, 1)
    tiles = L.lib.vs_conv2d_stat_rows(d, L.ConvTrain())
    assert tiles > 0
    xd, wd = to_nhwc(x, 1), w_krsc(wt, 1)
    nb = 16

    def run(kind):
        t = L.ConvTrain()
        if kind == "bins":
            acc = torch.zeros((nb, 2, cout), dtype=torch.int64, device=DEV)
            t.stats_bins, t.stats_nb = acc.data_ptr(), nb
        else:
            acc = _nan((tiles, 2, cout))
            t.stats_partial = acc.data_ptr()
        got = L.lib.vs_conv2d_train_variant(d, t)
        assert got == variant, f"this launch selects kernel variant {got}, not the ring kernel {variant} the batch-32 step runs"
        y = _nan((n, h, h, cout), torch.bfloat16)
        L.check(L.lib.vs_conv2d_train(d, L.ptr(xd), None, L.ptr(wd), None, L.ptr(y), None, ctypes.byref(t), None))
        torch.cuda.synchronize()
        tot = acc.sum(0).cpu().double() if kind == "bins" else acc.double().sum(0).cpu()
        if kind == "bins":
            tot = torch.stack([tot[0] / L.lib.vs_stat_scale(0), tot[1] / L.lib.vs_stat_scale(1)])
        return y, acc, tot

    y, bins, (s1, s2) = run(stats)
    out = y.view(-1, cout).double().cpu()
    assert torch.isfinite(out).all()
    assert torch.allclose(out, ref, **tol(1, ref.abs().max().item())), (out - ref).abs().max()
    figures, curve, _ = ring_variance_figures(h, cin, cout, s1, s2, tiles, stats == "bins", n)
    if stats == "bins":
        # the same tiles' fp32 sums as partial rows (the launch is deterministic): each atomic add rounded its value to the nearest
        # integer of 2^24 / 2^16, so the two totals differ by at most half such a unit per tile - the sharp check of the bins themselves,
        # free of the accumulators' error that dominates the bound above
        _, _, (r1, r2) = run("rows")
        figures += [("bins against rows sum", worst((s1 - r1).abs(), torch.tensor(tiles * 2.0 ** -25, dtype=torch.float64))),
                    ("bins against rows sumsq", worst((s2 - r2).abs(), torch.tensor(tiles * 2.0 ** -17, dtype=torch.float64)))]
        figures += ring_apply_figures(h, cin, cout, y, bins, nb, tiles, n)
    return figures, curve
