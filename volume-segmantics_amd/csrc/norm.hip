// BatchNorm2d on NHWC activations viewed as [rows = N*H*W][C] (gfx950).  HBM-bound streaming kernels:
// 16-byte loads per lane, per-channel reductions kept in registers across a row loop, combined
// through LDS, written as per-block partials and finalised in fp64 in a fixed order (bitwise
// reproducible - no float atomics).
//
// Semantics = torch.nn.BatchNorm2d defaults used by smp/torchvision: eps 1e-5, momentum 0.1,
// biased variance for normalisation, unbiased variance for the running estimate.
#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "common.h"
#include "prof.h"

namespace {

constexpr int kVec = 8;  // channels per thread (C is always a multiple of 8 in this network)
constexpr int kMaxBlocks = 2048;
constexpr int kU = 4;    // rows per trip of the streaming kernels (loads of a trip are issued together)
static int g_bn_blocks = getenv("VS_BN_BLOCKS") ? atoi(getenv("VS_BN_BLOCKS")) : 1024;
static int g_bn_iters = getenv("VS_BN_ITERS") ? atoi(getenv("VS_BN_ITERS")) : 4;

struct RowMap {
    int cv;       // channel vectors per row = C / 8
    int rpb;      // rows processed per block iteration = 256 / cv
    int nblocks;  // grid size
    int64_t rows_per_block;
};

RowMap make_rowmap(int64_t rows, int c, int max_blocks = 0) {
    RowMap m;
    m.cv = c / kVec;
    if (m.cv > 256) m.cv = 256;  // C <= 2048
    m.rpb = 256 / m.cv;
    int64_t iters = (rows + m.rpb - 1) / m.rpb;
    int64_t nb = (iters + g_bn_iters - 1) / g_bn_iters;  // >= g_bn_iters iterations per block when possible
    if (nb > g_bn_blocks) nb = g_bn_blocks;
    if (max_blocks > 0 && nb > max_blocks) nb = max_blocks;
    if (nb < 1) nb = 1;
    m.nblocks = (int)nb;
    int64_t ipb = (iters + nb - 1) / nb;
    m.rows_per_block = ipb * m.rpb;
    return m;
}

// ---- prefetched first trip (the `bn_prefetch` option, PF forms of the sweeps below) ----------------------------------------------
// A deep-layer workgroup runs exactly one trip, and in front of it up to two more dependent memory rounds: the statistics rows it
// sums itself, then the per-channel parameters.  None of the trip's row loads depends on those, so the PF forms issue them (and the
// parameter loads) first and keep the rows in their storage format across the prologue: three round trips become one.  A plain
// __syncthreads() is a bare s_barrier here (no LDS-DMA in flight): ordinary loads stay in flight across it.
// 8 consecutive elements in their storage format (4 registers for the 16-bit types) until they are used: unpack8(ld8raw(p)) is ld8(p)
template <typename T> struct Raw8 { uint4 u; };
template <> struct Raw8<float> { float4 a, b; };
template <typename T> __device__ __forceinline__ Raw8<T> ld8raw(const T* p) { return Raw8<T>{*reinterpret_cast<const uint4*>(p)}; }
template <> __device__ __forceinline__ Raw8<float> ld8raw<float>(const float* p) { return Raw8<float>{ld4(p), ld4(p + 4)}; }
__device__ __forceinline__ void unpack8(const Raw8<bf16_t>& r, float* o) {
    o[0] = __uint_as_float(r.u.x << 16); o[1] = __uint_as_float(r.u.x & 0xffff0000u);
    o[2] = __uint_as_float(r.u.y << 16); o[3] = __uint_as_float(r.u.y & 0xffff0000u);
    o[4] = __uint_as_float(r.u.z << 16); o[5] = __uint_as_float(r.u.z & 0xffff0000u);
    o[6] = __uint_as_float(r.u.w << 16); o[7] = __uint_as_float(r.u.w & 0xffff0000u);
}
__device__ __forceinline__ void unpack8(const Raw8<f16_t>& r, float* o) {
    const float2 a = unpack_f16(r.u.x), b = unpack_f16(r.u.y), c = unpack_f16(r.u.z), d = unpack_f16(r.u.w);
    o[0] = a.x; o[1] = a.y; o[2] = b.x; o[3] = b.y; o[4] = c.x; o[5] = c.y; o[6] = d.x; o[7] = d.y;
}
__device__ __forceinline__ void unpack8(const Raw8<float>& r, float* o) {
    o[0] = r.a.x; o[1] = r.a.y; o[2] = r.a.z; o[3] = r.a.w; o[4] = r.b.x; o[5] = r.b.y; o[6] = r.b.z; o[7] = r.b.w;
}
// four statistics of partial row r (zeros past the last row) by an UNCONDITIONAL load: a row past the end re-reads row `fb` and is
// masked afterwards - around a conditional load hipcc branches and waits, one dependent round per row instead of one per four rows
__device__ __forceinline__ float4 partial_row4(const float* __restrict__ partial, int r, int fb, int nparts, int stride, int col) {
    const float4 t = *reinterpret_cast<const float4*>(partial + (size_t)(r < nparts ? r : fb) * stride + col * 4);
    return r < nparts ? t : make_float4(0.f, 0.f, 0.f, 0.f);
}
// element offsets of the kU rows of the trip that starts at row rb: a row past r1 re-reads row `fb` (an existing one) and is masked
// at use.  The row loops pass fb = rb; the prefetch, which runs before anything is known to be in range, passes live = false for a
// thread without a first row (idle lane, empty or ragged block) and reads row 0 - no thread ever forms an out-of-range address.
__device__ __forceinline__ void trip_offsets(int64_t rb, int64_t r1, bool live, int rpb, int c, int cvi, size_t (&o)[kU], bool (&ok)[kU]) {
    const int64_t fb = live ? rb : 0;
#pragma unroll
    for (int u = 0; u < kU; ++u) {
        const int64_t r = rb + (int64_t)u * rpb;
        ok[u] = live && r < r1;
        o[u] = (size_t)(ok[u] ? r : fb) * c + cvi * kVec;
    }
}

// ---- building blocks of the reductions ---------------------------------------------------------
// The tail of the two partial-sum kernels: the 256 threads' 8-channel sums (s, q) become this block's partial row [2][c].  Thread
// ch < cv * 8 adds the rpb row lanes of its channel in lane order (fp32, fixed order).
__device__ __forceinline__ void fold_block_sums(const float (&s)[kVec], const float (&q)[kVec], const RowMap& m, int c, float* __restrict__ partial) {
    __shared__ float red[2][256][kVec + 1];
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < kVec; ++k) { red[0][tid][k] = s[k]; red[1][tid][k] = q[k]; }
    __syncthreads();
    for (int ch = tid; ch < m.cv * kVec; ch += 256) {
        const int g = ch / kVec, k = ch % kVec;
        float a = 0.f, b = 0.f;
        for (int j = 0; j < m.rpb; ++j) { a += red[0][j * m.cv + g][k]; b += red[1][j * m.cv + g][k]; }
        partial[((size_t)blockIdx.x * 2 + 0) * c + ch] = a;
        partial[((size_t)blockIdx.x * 2 + 1) * c + ch] = b;
    }
}

// The fp64 sum over a few partial rows [nparts][2][c] inside a sweep (needs c <= 512 and 256 % (2 c / 4) == 0), by all 256 threads:
// thread (column of four statistics, row group) sums its rows with 16-byte loads, four in flight; the row groups meet in LDS in a
// fixed order (fp64 throughout: every workgroup forms the same numbers).  done(ch, s, q) gets the two totals of channel ch.
template <typename F>
__device__ __forceinline__ void sum_partial_rows_f64(const float* __restrict__ partial, int nparts, int c, F&& done) {
    __shared__ double dsum[4096];                                  // [RG][2 c]
    const int tid = threadIdx.x;
    const int cols = (2 * c) / 4, RG = 256 / cols, col = tid % cols, rg = tid / cols;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    for (int r = rg; r < nparts; r += 4 * RG) {
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = partial_row4(partial, r + u * RG, r, nparts, 2 * c, col);
#pragma unroll
        for (int u = 0; u < 4; ++u) { a0 += (double)v[u].x; a1 += (double)v[u].y; a2 += (double)v[u].z; a3 += (double)v[u].w; }
    }
    double* d = dsum + (size_t)rg * 2 * c + col * 4;
    d[0] = a0; d[1] = a1; d[2] = a2; d[3] = a3;
    __syncthreads();
    for (int ch = tid; ch < c; ch += 256) {
        double s = 0.0, q = 0.0;
        for (int g2 = 0; g2 < RG; ++g2) { s += dsum[(size_t)g2 * 2 * c + ch]; q += dsum[(size_t)g2 * 2 * c + c + ch]; }
        done(ch, s, q);
    }
}

// The statistics finish of channel ch: mean, clamped biased variance and invstd from the fp64 sums of (x - K) and (x - K)^2 over n
// rows, and, where publish, mean / invstd for the backward pass and the running update (unbiased variance).  K is the shift of
// bn_stats_partial's sums; the unshifted sources pass 0.0, and dm + 0.0 is dm to the bit (a sum that starts from +0.0 is never -0.0).
struct MeanInvstd { float mean, invstd; };
__device__ __forceinline__ MeanInvstd finish_stats(double s, double q, int64_t n, float eps, float momentum, double K, int ch, bool publish,
                                                   float* mean, float* invstd, float* running_mean, float* running_var) {
    const double dm = s / (double)n;  // mean of (x - K)
    double var = q / (double)n - dm * dm;
    if (var < 0.0) var = 0.0;
    const double mu = dm + K;
    const MeanInvstd r{(float)mu, (float)(1.0 / sqrt(var + (double)eps))};
    if (publish) {
        mean[ch] = r.mean;
        invstd[ch] = r.invstd;
        if (running_mean) {
            const double unbiased = n > 1 ? var * (double)n / (double)(n - 1) : var;
            running_mean[ch] = (float)((1.0 - momentum) * (double)running_mean[ch] + momentum * mu);
            running_var[ch] = (float)((1.0 - momentum) * (double)running_var[ch] + momentum * unbiased);
        }
    }
    return r;
}

// ---- forward statistics ------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void bn_stats_partial(const T* __restrict__ x, int64_t rows, int c, RowMap m,
                                                      float* __restrict__ partial) {
    const int tid = threadIdx.x;
    const int cvi = tid % m.cv, rl = tid / m.cv;
    float s[kVec], q[kVec], sh[kVec];
#pragma unroll
    for (int k = 0; k < kVec; ++k) s[k] = q[k] = 0.f;
    // shifted sums: K = first row of the tensor (same for every block) keeps E[(x-K)^2] - E[x-K]^2 free of
    // catastrophic cancellation when |mean| >> std (few samples per channel in the deep layers)
    ld8(x + cvi * kVec, sh);
    const int64_t r0 = (int64_t)blockIdx.x * m.rows_per_block;
    const int64_t r1 = min(rows, r0 + m.rows_per_block);
    if (rl < m.rpb) {
        for (int64_t r = r0 + rl; r < r1; r += m.rpb) {
            float v[kVec];
            ld8(x + r * c + cvi * kVec, v);
#pragma unroll
            for (int k = 0; k < kVec; ++k) { const float d = v[k] - sh[k]; s[k] += d; q[k] += d * d; }
        }
    }
    fold_block_sums(s, q, m, c, partial);
}

// one wave per channel: lanes stride over the per-block partials, fp64 butterfly reduction (fixed order)
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// one 256-thread block per channel: threads stride over the per-block partials, fp64 wave butterflies, 4 waves meet in LDS
__device__ __forceinline__ void block_sum2_f64(double& s, double& q) {
    __shared__ double red[2][4];
    s = wave_sum_f64(s);
    q = wave_sum_f64(q);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { red[0][wave] = s; red[1][wave] = q; }
    __syncthreads();
    s = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    q = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
}

// thread t sums partial rows t, t+256, .. of channel ch (both statistics) in that order; the loads of four rows are issued
// together so the kernel pays one memory round trip per four rows instead of one per row (these kernels are pure latency)
__device__ __forceinline__ void strided_sum2_f64(const float* __restrict__ partial, int nblocks, int c, int ch, double& s, double& q) {
    for (int b = threadIdx.x; b < nblocks; b += 4 * 256) {
        float a[4], d[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int r = b + u * 256;
            const bool ok = r < nblocks;
            a[u] = ok ? partial[((size_t)r * 2 + 0) * c + ch] : 0.f;
            d[u] = ok ? partial[((size_t)r * 2 + 1) * c + ch] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) { s += (double)a[u]; q += (double)d[u]; }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void bn_stats_finalize(const float* __restrict__ partial, const T* __restrict__ x,
                                                         int nblocks, int c, int64_t rows, float eps, float momentum,
                                                         float* mean, float* invstd, float* running_mean,
                                                         float* running_var) {
    const int ch = blockIdx.x;
    double s = 0.0, q = 0.0;
    strided_sum2_f64(partial, nblocks, c, ch, s, q);
    block_sum2_f64(s, q);
    if (threadIdx.x != 0) return;
    finish_stats(s, q, rows, eps, momentum, x ? (double)Elem<T>::ld(x + ch) : 0.0, ch, true, mean, invstd, running_mean, running_var);
}

// ---- forward apply -----------------------------------------------------------------------------
// The rows of one trip: normalise, add the residual, ReLU, guarded store.  a = invstd * gamma, b = beta, mu = mean of the thread's
// eight channels; rv is read only where res is given.
template <typename T>
__device__ __forceinline__ void bn_fwd_rows(float (&v)[kU][kVec], const float (&rv)[kU][kVec], const float (&a)[kVec], const float (&b)[kVec],
                                            const float (&mu)[kVec], const bool (&ok)[kU], const size_t (&o)[kU], const T* __restrict__ res,
                                            int relu, T* __restrict__ y) {
#pragma unroll
    for (int u = 0; u < kU; ++u) {
#pragma unroll
        for (int k = 0; k < kVec; ++k) v[u][k] = (v[u][k] - mu[k]) * a[k] + b[k];
        if (res) {
#pragma unroll
            for (int k = 0; k < kVec; ++k) v[u][k] += rv[u][k];
        }
        if (relu) {
#pragma unroll
            for (int k = 0; k < kVec; ++k) v[u][k] = fmaxf(v[u][k], 0.f);
        }
        if (ok[u]) st8(y + o[u], v[u]);
    }
}

// A thread's trips from row rb on.  kU rows per trip with every load issued before the first use: one 16-byte load in flight per
// thread left these sweeps latency-bound at ~2.5 TB/s (a trip per ~1 us memory round trip)
template <typename T>
__device__ __forceinline__ void bn_fwd_sweep(int64_t rb, int64_t r1, const RowMap& m, int c, int cvi, const T* __restrict__ x,
                                             const T* __restrict__ res, int relu, T* __restrict__ y, const float (&a)[kVec],
                                             const float (&b)[kVec], const float (&mu)[kVec]) {
    for (; rb < r1; rb += (int64_t)kU * m.rpb) {
        float v[kU][kVec], rv[kU][kVec];
        size_t o[kU];
        bool ok[kU];
        trip_offsets(rb, r1, true, m.rpb, c, cvi, o, ok);
#pragma unroll
        for (int u = 0; u < kU; ++u) ld8(x + o[u], v[u]);
        if (res) {
#pragma unroll
            for (int u = 0; u < kU; ++u) ld8(res + o[u], rv[u]);
        }
        bn_fwd_rows(v, rv, a, b, mu, ok, o, res, relu, y);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void bn_apply_kernel(const T* __restrict__ x, const float* __restrict__ mean,
                                                     const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, const T* __restrict__ res, int relu,
                                                     T* __restrict__ y, int64_t rows, int c, RowMap m) {
    const int tid = threadIdx.x;
    const int cvi = tid % m.cv, rl = tid / m.cv;
    if (rl >= m.rpb) return;
    float a[kVec], b[kVec], mu[kVec];
#pragma unroll
    for (int k = 0; k < kVec; ++k) {
        const int ch = cvi * kVec + k;
        a[k] = invstd[ch] * gamma[ch];
        b[k] = beta[ch];
        mu[k] = mean[ch];
    }
    const int64_t r0 = (int64_t)blockIdx.x * m.rows_per_block;
    const int64_t r1 = min(rows, r0 + m.rows_per_block);
    bn_fwd_sweep(r0 + rl, r1, m, c, cvi, x, res, relu, y, a, b, mu);
}

// Same, with the statistics finalised INSIDE the kernel: when the producing convolution left only a few partial rows
// (<= 64: the 16x16 / 8x8-pixel layers), every workgroup sums them itself (fp64, rows in order) instead of waiting for a
// separate finalise launch - ~1.5 us of redundant work per workgroup against ~7 us of launch + drain on the critical path.
// Workgroup 0 also publishes mean / invstd for the backward pass and updates the running statistics.
// FIXED: `partial` holds nparts rows of 64-bit fixed-point bins ([row][2][c]: sum x * 2^24, sum x^2 * 2^16, accumulated by atomic adds
// in the producing convolution's epilogue - ConvParams::stats_bins) instead of fp32 partial rows
// PF decides only where trip 0's loads are issued.  PF = true: its rows (x, residual) in their storage format and gamma / beta are
// loaded BEFORE the statistics prologue (see Raw8 above), trip 0 is unpacked from registers and the loop starts at trip 1.
// PF = false: the same sweep without the early loads - the loop starts at trip 0.  It is the reference form of
// tests/test_hip_bn_prefetch.py and the other arm of the A/B (option bn_prefetch)
template <typename T, bool FIXED, bool PF>
__global__ __launch_bounds__(256) void bn_apply_inline_kernel(const T* __restrict__ x, const float* __restrict__ partial, int nparts,
                                                            float eps, float momentum, float* __restrict__ mean,
                                                            float* __restrict__ invstd, float* __restrict__ running_mean,
                                                            float* __restrict__ running_var, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, const T* __restrict__ res, int relu,
                                                            T* __restrict__ y, int64_t rows, int c, RowMap m, int64_t stat_rows) {
    extern __shared__ float s_stat[];   // [2][c]: mean, invstd
    const int tid = threadIdx.x;
    const int cvi = tid % m.cv, rl = tid / m.cv;
    const int64_t r0 = (int64_t)blockIdx.x * m.rows_per_block;
    const int64_t r1 = min(rows, r0 + m.rows_per_block);
    Raw8<T> px[PF ? kU : 1], pr[PF ? kU : 1];
    float pg[PF ? kVec : 1], pb[PF ? kVec : 1];
    if constexpr (PF) {
        size_t o[kU];
        bool ok[kU];
        trip_offsets(r0 + rl, r1, rl < m.rpb && r0 + rl < r1, m.rpb, c, cvi, o, ok);
#pragma unroll
        for (int u = 0; u < kU; ++u) px[u] = ld8raw(x + o[u]);
        if (res) {
#pragma unroll
            for (int u = 0; u < kU; ++u) pr[u] = ld8raw(res + o[u]);
        }
#pragma unroll
        for (int k = 0; k < kVec; ++k) { pg[k] = gamma[cvi * kVec + k]; pb[k] = beta[cvi * kVec + k]; }
    }
    if (stat_rows <= 0) stat_rows = rows;        // (the sums may describe more rows than this rank sweeps: cross-rank statistics)
    auto finish = [&](int ch, double s, double q) {
        const MeanInvstd r = finish_stats(s, q, stat_rows, eps, momentum, 0.0, ch, blockIdx.x == 0, mean, invstd, running_mean, running_var);
        s_stat[ch] = r.mean;
        s_stat[c + ch] = r.invstd;
    };
    if constexpr (FIXED) {
        // integer sums: any summation order gives the same bits, so all 256 threads share the rows - thread (value column, row
        // group) adds its rows with the loads independent of each other, the row groups meet in LDS
        const long long* bins = reinterpret_cast<const long long*>(partial);
        const int nv = 2 * c;                           // values per bin row: [2][c]
        long long* isum = reinterpret_cast<long long*>(s_stat + 2 * c);     // max(256, nv) entries behind the statistics (dynamic LDS:
                                                                             // a static 32 KB array would cap the sweep's occupancy)
        if (nv <= 256) {
            const int RG = 256 / nv, col = tid % nv, rg = tid / nv;
            long long acc = 0;
            if (rg < RG) {
#pragma unroll 8
                for (int r = rg; r < nparts; r += RG) acc += bins[(size_t)r * nv + col];
                isum[rg * nv + col] = acc;
            }
            __syncthreads();
            for (int ch = tid; ch < c; ch += 256) {
                long long sv = 0, qv = 0;
                for (int g2 = 0; g2 < RG; ++g2) { sv += isum[g2 * nv + ch]; qv += isum[g2 * nv + c + ch]; }
                finish(ch, (double)sv * (1.0 / kStatScale1), (double)qv * (1.0 / kStatScale2));
            }
        } else {
            for (int col = tid; col < nv; col += 256) {
                long long acc = 0;
#pragma unroll 8
                for (int r = 0; r < nparts; ++r) acc += bins[(size_t)r * nv + col];
                isum[col] = acc;
            }
            __syncthreads();
            for (int ch = tid; ch < c; ch += 256) finish(ch, (double)isum[ch] * (1.0 / kStatScale1), (double)isum[c + ch] * (1.0 / kStatScale2));
        }
    } else if (c <= 512 && 256 % ((2 * c) / 4) == 0) {
        sum_partial_rows_f64(partial, nparts, c, finish);
    } else {
        for (int ch = tid; ch < c; ch += 256) {
            double s = 0.0, q = 0.0;
#pragma unroll 8
            for (int r = 0; r < nparts; ++r) {
                s += (double)partial[((size_t)r * 2 + 0) * c + ch];
                q += (double)partial[((size_t)r * 2 + 1) * c + ch];
            }
            finish(ch, s, q);
        }
    }
    __syncthreads();
    if (rl >= m.rpb) return;
    float a[kVec], b[kVec], mu[kVec];
#pragma unroll
    for (int k = 0; k < kVec; ++k) {
        const int ch = cvi * kVec + k;
        if constexpr (PF) { a[k] = s_stat[c + ch] * pg[k]; b[k] = pb[k]; }
        else { a[k] = s_stat[c + ch] * gamma[ch]; b[k] = beta[ch]; }
        mu[k] = s_stat[ch];
    }
    int64_t rb = r0 + rl;
    if constexpr (PF) {      // trip 0 from the prefetched registers
        float v[kU][kVec], rv[kU][kVec];
        size_t o[kU];
        bool ok[kU];
        trip_offsets(rb, r1, rb < r1, m.rpb, c, cvi, o, ok);
#pragma unroll
        for (int u = 0; u < kU; ++u) unpack8(px[u], v[u]);
        if (res) {
#pragma unroll
            for (int u = 0; u < kU; ++u) unpack8(pr[u], rv[u]);
        }
        bn_fwd_rows(v, rv, a, b, mu, ok, o, res, relu, y);
        rb += (int64_t)kU * m.rpb;
    }
    bn_fwd_sweep(rb, r1, m, c, cvi, x, res, relu, y, a, b, mu);
}

// ---- backward ----------------------------------------------------------------------------------
// relu mask of one row: from the stored activation y, or (RECOMPUTE) recomputed as (x - mean) * invstd * gamma + beta > 0
// (bit-identical to the forward's expression; only valid for units without a residual input).  ga = invstd * gamma, be = beta.
template <bool RECOMPUTE>
__device__ __forceinline__ void bn_bwd_mask(float (&g)[kVec], const float (&xv)[kVec], const float (&yv)[kVec], const float (&mu)[kVec],
                                            const float (&ga)[RECOMPUTE ? kVec : 1], const float (&be)[RECOMPUTE ? kVec : 1]) {
    if constexpr (!RECOMPUTE) {
#pragma unroll
        for (int k = 0; k < kVec; ++k) g[k] = yv[k] > 0.f ? g[k] : 0.f;
    } else {
#pragma unroll
        for (int k = 0; k < kVec; ++k) g[k] = ((xv[k] - mu[k]) * ga[k] + be[k]) > 0.f ? g[k] : 0.f;
    }
}

// per-channel values of the backward rows for the thread's eight channels: gi = gamma * invstd, db = dbeta / n, dg = dgamma / n
template <bool RECOMPUTE>
struct BwdCoef {
    float mu[kVec], is[kVec], gi[kVec], db[kVec], dg[kVec], ga[RECOMPUTE ? kVec : 1], be[RECOMPUTE ? kVec : 1];
};

// The rows of one trip: mask, dres = the masked gradient, dx.  yv has one row where the mask is not read from y.
// RELU is a compile-time constant (std::true_type / std::false_type) where the mask is read from y, and the run-time flag where it is
// recomputed: see the sweep of bn_bwd_apply.
template <typename T, bool RECOMPUTE, typename RELU>
__device__ __forceinline__ void bn_bwd_rows(float (&g)[kU][kVec], const float (&xv)[kU][kVec], const float (&yv)[RECOMPUTE ? 1 : kU][kVec],
                                            const BwdCoef<RECOMPUTE>& k8, const bool (&ok)[kU], const size_t (&o)[kU], T* __restrict__ dres,
                                            T* __restrict__ dx, RELU relu) {
#pragma unroll
    for (int u = 0; u < kU; ++u) {
        if (!ok[u]) continue;
        if (relu) bn_bwd_mask<RECOMPUTE>(g[u], xv[u], yv[RECOMPUTE ? 0 : u], k8.mu, k8.ga, k8.be);
        if (dres) st8(dres + o[u], g[u]);
        float o8[kVec];
#pragma unroll
        for (int k = 0; k < kVec; ++k) o8[k] = k8.gi[k] * (g[u][k] - k8.db[k] - (xv[u][k] - k8.mu[k]) * k8.is[k] * k8.dg[k]);
        st8(dx + o[u], o8);
    }
}

template <typename T, bool RECOMPUTE>
__global__ __launch_bounds__(256) void bn_bwd_partial(const T* __restrict__ dy, const T* __restrict__ y,
                                                    const T* __restrict__ x, const float* __restrict__ mean,
                                                    const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                    const float* __restrict__ beta, int relu, int64_t rows, int c,
                                                    RowMap m, float* __restrict__ partial) {
    const int tid = threadIdx.x;
    const int cvi = tid % m.cv, rl = tid / m.cv;
    float s[kVec], q[kVec], mu[kVec], is[kVec], ga[RECOMPUTE ? kVec : 1], be[RECOMPUTE ? kVec : 1];
#pragma unroll
    for (int k = 0; k < kVec; ++k) {
        s[k] = q[k] = 0.f;
        mu[k] = mean[cvi * kVec + k];
        is[k] = invstd[cvi * kVec + k];
        if constexpr (RECOMPUTE) {
            ga[k] = invstd[cvi * kVec + k] * gamma[cvi * kVec + k];
            be[k] = beta[cvi * kVec + k];
        }
    }
    const int64_t r0 = (int64_t)blockIdx.x * m.rows_per_block;
    const int64_t r1 = min(rows, r0 + m.rows_per_block);
    if (rl < m.rpb) {
        for (int64_t rb = r0 + rl; rb < r1; rb += (int64_t)kU * m.rpb) {
            float g[kU][kVec], xv[kU][kVec], yv[RECOMPUTE ? 1 : kU][kVec];
            bool ok[kU];
#pragma unroll
            for (int u = 0; u < kU; ++u) {       // all loads of the trip first
                const int64_t r = rb + (int64_t)u * m.rpb;
                ok[u] = r < r1;
                const size_t o = (size_t)(ok[u] ? r : rb) * c + cvi * kVec;
                ld8(dy + o, g[u]);
                ld8(x + o, xv[u]);
                if constexpr (!RECOMPUTE) {
                    if (relu) ld8(y + o, yv[u]);
                }
            }
#pragma unroll
            for (int u = 0; u < kU; ++u) {       // rows in order: the sums are the ones the one-row-per-trip loop formed
                if (!ok[u]) continue;
                if (relu) bn_bwd_mask<RECOMPUTE>(g[u], xv[u], yv[RECOMPUTE ? 0 : u], mu, ga, be);
#pragma unroll
                for (int k = 0; k < kVec; ++k) { s[k] += g[u][k]; q[k] += g[u][k] * (xv[u][k] - mu[k]) * is[k]; }
            }
        }
    }
    fold_block_sums(s, q, m, c, partial);
}

__global__ __launch_bounds__(256) void bn_bwd_finalize(const float* __restrict__ partial, int nblocks, int c,
                                                       float* dgamma, float* dbeta) {
    const int ch = blockIdx.x;
    double s = 0.0, q = 0.0;
    strided_sum2_f64(partial, nblocks, c, ch, s, q);
    block_sum2_f64(s, q);
    if (threadIdx.x == 0) { dbeta[ch] = (float)s; dgamma[ch] = (float)q; }
}

// The apply sweep of the backward: dx (and dres) from dgamma / dbeta, which bn_bwd_finalize left or (INLINE) the sweep sums itself.
// INLINE: the reduction's partial rows (few: <= 64) are summed by every workgroup itself (fp64, fixed order - the numbers
// bn_bwd_finalize forms); workgroup 0 publishes dgamma / dbeta.  One launch and one dependent phase fewer per unit.
// PF decides only where trip 0's loads are issued.  PF = true: its rows (dy, x, y) in their storage format and mean / invstd /
// gamma / beta are loaded before the prologue (INLINE: the partial-row sum; otherwise the dbeta / dgamma loads and their products),
// trip 0 is unpacked from registers and the loop starts at trip 1.  PF = false: the same sweep without the early loads.
template <typename T, bool RECOMPUTE, bool INLINE, bool PF>
__global__ __launch_bounds__(256) void bn_bwd_apply(const T* __restrict__ dy, const T* __restrict__ y,
                                                  const T* __restrict__ x, const float* __restrict__ mean,
                                                  const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                  const float* __restrict__ beta, float* __restrict__ dgamma,
                                                  float* __restrict__ dbeta, int relu, T* __restrict__ dx,
                                                  T* __restrict__ dres, int64_t rows, int c, RowMap m,
                                                  const float* __restrict__ partial, int nparts, int64_t stat_rows) {
    const int tid = threadIdx.x;
    const int cvi = tid % m.cv, rl = tid / m.cv;
    const int64_t r0 = (int64_t)blockIdx.x * m.rows_per_block;
    const int64_t r1 = min(rows, r0 + m.rows_per_block);
    constexpr int NY = RECOMPUTE ? 1 : kU;
    Raw8<T> pdy[PF ? kU : 1], px[PF ? kU : 1], py[PF ? NY : 1];
    float pmu[PF ? kVec : 1], pis[PF ? kVec : 1], pga[PF ? kVec : 1], pbe[PF && RECOMPUTE ? kVec : 1];
    if constexpr (PF) {
        size_t o[kU];
        bool ok[kU];
        trip_offsets(r0 + rl, r1, rl < m.rpb && r0 + rl < r1, m.rpb, c, cvi, o, ok);
#pragma unroll
        for (int u = 0; u < kU; ++u) { pdy[u] = ld8raw(dy + o[u]); px[u] = ld8raw(x + o[u]); }
        if constexpr (!RECOMPUTE) {
            if (relu) {
#pragma unroll
                for (int u = 0; u < kU; ++u) py[u] = ld8raw(y + o[u]);
            }
        }
#pragma unroll
        for (int k = 0; k < kVec; ++k) {
            const int ch = cvi * kVec + k;
            pmu[k] = mean[ch]; pis[k] = invstd[ch]; pga[k] = gamma[ch];
            if constexpr (RECOMPUTE) pbe[k] = beta[ch];
        }
    }
    __shared__ float s_coef[INLINE ? 2 * 512 : 1];                     // [0, c): dbeta, [c, 2 c): dgamma
    if constexpr (INLINE) {
        sum_partial_rows_f64(partial, nparts, c, [&](int ch, double s, double q) {
            s_coef[ch] = (float)s;
            s_coef[c + ch] = (float)q;
            if (blockIdx.x == 0) { dbeta[ch] = (float)s; dgamma[ch] = (float)q; }
        });
        __syncthreads();
    }
    if (rl >= m.rpb) return;
    const float inv_m = 1.0f / (float)(stat_rows > 0 ? stat_rows : rows);   // (stat_rows: the sums cover the rows of every rank)
    BwdCoef<RECOMPUTE> k8;
#pragma unroll
    for (int k = 0; k < kVec; ++k) {
        const int ch = cvi * kVec + k;
        if constexpr (PF) { k8.mu[k] = pmu[k]; k8.is[k] = pis[k]; k8.gi[k] = pga[k] * pis[k]; }
        else { k8.mu[k] = mean[ch]; k8.is[k] = invstd[ch]; k8.gi[k] = gamma[ch] * invstd[ch]; }
        if constexpr (INLINE) { k8.db[k] = s_coef[ch] * inv_m; k8.dg[k] = s_coef[c + ch] * inv_m; }
        else { k8.db[k] = dbeta[ch] * inv_m; k8.dg[k] = dgamma[ch] * inv_m; }
        if constexpr (RECOMPUTE) {
            if constexpr (PF) { k8.be[k] = pbe[k]; k8.ga[k] = pis[k] * pga[k]; }
            else { k8.be[k] = beta[ch]; k8.ga[k] = invstd[ch] * gamma[ch]; }
        }
    }
    // Where the mask is read from y, the sweep exists in two versions, with and without the ReLU mask (relu_c a compile-time constant):
    // a `relu` test inside the unrolled row loop makes hipcc branch around every y load and wait for each one (four dependent rounds
    // per trip instead of one).  The recomputed mask loads nothing, and there the test stays in the row loop (relu_c the run-time
    // flag): hoisted, the fp32 sweep takes 138 registers instead of 128 and loses a wave per SIMD.
    auto sweep = [&](auto relu_c) {
        int64_t rb = r0 + rl;
        if constexpr (PF) {      // trip 0 from the prefetched registers
            float g[kU][kVec], xv[kU][kVec], yv[NY][kVec];
            size_t o[kU];
            bool ok[kU];
            trip_offsets(rb, r1, rb < r1, m.rpb, c, cvi, o, ok);
#pragma unroll
            for (int u = 0; u < kU; ++u) {
                unpack8(pdy[u], g[u]);
                unpack8(px[u], xv[u]);
                if constexpr (!RECOMPUTE) { if (relu_c) unpack8(py[u], yv[u]); }
            }
            bn_bwd_rows<T, RECOMPUTE>(g, xv, yv, k8, ok, o, dres, dx, relu_c);
            rb += (int64_t)kU * m.rpb;
        }
        for (; rb < r1; rb += (int64_t)kU * m.rpb) {
            float g[kU][kVec], xv[kU][kVec], yv[NY][kVec];
            size_t o[kU];
            bool ok[kU];
            trip_offsets(rb, r1, true, m.rpb, c, cvi, o, ok);
#pragma unroll
            for (int u = 0; u < kU; ++u) {       // all loads of the trip first
                ld8(dy + o[u], g[u]);
                ld8(x + o[u], xv[u]);
                if constexpr (!RECOMPUTE) { if (relu_c) ld8(y + o[u], yv[u]); }
            }
            bn_bwd_rows<T, RECOMPUTE>(g, xv, yv, k8, ok, o, dres, dx, relu_c);
        }
    };
    if constexpr (RECOMPUTE) sweep(relu != 0);
    else if (relu) sweep(std::true_type{});
    else sweep(std::false_type{});
}

__global__ void bn_fold_kernel(const float* gamma, const float* beta, const float* rm, const float* rv, float eps,
                               float* scale, float* shift, int c) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= c) return;
    const float s = gamma[i] / sqrtf(rv[i] + eps);
    scale[i] = s;
    shift[i] = beta[i] - rm[i] * s;
}

// ---- host side ---------------------------------------------------------------------------------
// one sweep launch: m.nblocks workgroups of 256 threads, every argument converted to the kernel's parameter type by static_cast (untyped
// tensors to T*, null to a typed null): an argument in the wrong place, or one that would lose its const, does not compile
template <typename... P, typename... A>
int launch_sweep(void (*kernel)(P...), const RowMap& m, size_t lds, hipStream_t s, A... args) {
    static_assert(sizeof...(P) == sizeof...(A), "one argument per kernel parameter");
    hipLaunchKernelGGL(kernel, dim3(m.nblocks), dim3(256), lds, s, static_cast<P>(args)...);
    VS_LAUNCH_CHECK();
    return VS_OK;
}

// what every kernel of this file needs of the channel count: 8 channels per thread, at most 256 such threads per row
int bn_channels_ok(int c, const char* what) {
    VS_REQUIRE(c % kVec == 0 && c <= 2048, "%s: unsupported channel count %d", what, c);
    return VS_OK;
}

template <typename T>
int stats_t(const void* x, int64_t rows, int c, float eps, float momentum, float* mean, float* invstd, float* rm,
            float* rv, float* ws, hipStream_t s) {
    RowMap m = make_rowmap(rows, c);
    if (const int rc = launch_sweep(bn_stats_partial<T>, m, 0, s, x, rows, c, m, ws)) return rc;
    hipLaunchKernelGGL(bn_stats_finalize<T>, dim3(c), dim3(256), 0, s, ws, (const T*)x, m.nblocks, c, rows, eps,
                       momentum, mean, invstd, rm, rv);
    VS_LAUNCH_CHECK();
    return VS_OK;
}

// which form of the sweeps a launch takes (read at launch time; 0 = the same sweeps without the early loads of the first trip)
bool bn_prefetch() { return vs_option("bn_prefetch") != 0; }
// The prefetch form of bn_bwd_apply holds the first trip beside the parameters: 170 registers against 120 for bf16 (fp32: 232 against
// 150; compiler figures, profiles/norm_refactor.txt), two workgroups per CU instead of four.  It takes the INLINE launches (11.7 ->
// 8.9 us median in the traced step) whose workgroups are all resident at once either way - the latency-bound deep layers.  The plain
// apply sweep measured no faster in that form (one hidden round, paid for with the occupancy) and keeps the form without it, as does
// bn_bwd_partial.
bool bn_bwd_prefetch(const RowMap& m) { return bn_prefetch() && m.nblocks <= 2 * device_cus(); }

// train-mode BN forward in ONE launch (few statistics rows): finalise + normalise.  `stats`: fp32 partial rows, or (FIXED) bins
template <bool FIXED>
int bn_apply_inline(int dtype, const void* x, const float* stats, int nstats, float eps, float momentum, float* mean, float* invstd,
                    float* running_mean, float* running_var, const float* gamma, const float* beta, const void* residual, int relu, void* y,
                    int64_t rows, int c, hipStream_t s, int64_t stat_rows) {
    if (const int rc = bn_channels_ok(c, "bn_apply")) return rc;
    VS_REQUIRE(!FIXED || nstats >= 1, "bn_apply: %d rows of bins", nstats);
    RowMap m = make_rowmap(rows, c);
    const size_t lds = 2 * (size_t)c * sizeof(float) + (FIXED ? (size_t)std::max(256, 2 * c) * sizeof(long long) : 0);
    const bool pf = bn_prefetch();
    VS_FOR_T(dtype, return launch_sweep(pf ? bn_apply_inline_kernel<T, FIXED, true> : bn_apply_inline_kernel<T, FIXED, false>, m, lds, s, x, stats, nstats,
                                        eps, momentum, mean, invstd, running_mean, running_var, gamma, beta, residual, relu, y, rows, c, m, stat_rows));
}

}  // namespace

// from the conv epilogue's partial rows
int launch_bn_apply_from_partials(int dtype, const void* x, const float* partial, int nparts, float eps, float momentum, float* mean,
                                  float* invstd, float* running_mean, float* running_var, const float* gamma, const float* beta,
                                  const void* residual, int relu, void* y, int64_t rows, int c, hipStream_t s) {
    return bn_apply_inline<false>(dtype, x, partial, nparts, eps, momentum, mean, invstd, running_mean, running_var, gamma, beta, residual, relu, y,
                                  rows, c, s, 0);
}

// from the conv epilogue's fixed-point bins
int launch_bn_apply_from_bins(int dtype, const void* x, const unsigned long long* bins, int nb, float eps, float momentum, float* mean,
                              float* invstd, float* running_mean, float* running_var, const float* gamma, const float* beta,
                              const void* residual, int relu, void* y, int64_t rows, int c, hipStream_t s, int64_t stat_rows) {
    return bn_apply_inline<true>(dtype, x, (const float*)bins, nb, eps, momentum, mean, invstd, running_mean, running_var, gamma, beta, residual, relu,
                                 y, rows, c, s, stat_rows);
}

namespace {
__global__ void zero_u64_kernel(unsigned long long* __restrict__ p, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) p[i] = 0ull;
}
}  // namespace
// (a kernel, not hipMemsetAsync: a recorded step stays a linear graph of kernel nodes)
int launch_zero_u64(unsigned long long* p, size_t n, hipStream_t s) {
    if (!n) return VS_OK;
    hipLaunchKernelGGL(zero_u64_kernel, dim3((unsigned)std::min<size_t>((n + 255) / 256, 2048)), dim3(256), 0, s, p, n);
    VS_LAUNCH_CHECK();
    return VS_OK;
}

int launch_bn_finalize_partials(const float* partial, int nparts, int c, int64_t rows, float eps, float momentum,
                                float* mean, float* invstd, float* running_mean, float* running_var, hipStream_t s) {
    hipLaunchKernelGGL(bn_stats_finalize<float>, dim3(c), dim3(256), 0, s, partial, (const float*)nullptr, nparts, c, rows, eps,
                       momentum, mean, invstd, running_mean, running_var);
    VS_LAUNCH_CHECK();
    return VS_OK;
}

namespace {
__global__ void bn_sync_pack_kernel(const float* __restrict__ dbeta, const float* __restrict__ dgamma, float* __restrict__ out, int c) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < c) { out[i] = dbeta[i]; out[c + i] = dgamma[i]; }
}
}  // namespace
// cross-rank sums for the BatchNorm-backward apply: this rank's (dbeta, dgamma) stay where the optimiser reads them (the gradient
// all-reduce averages those like every other gradient), a copy is summed over the ranks and feeds dx
static int bn_sync_sums(const BnSync& sy, const float* dgamma, const float* dbeta, int c, hipStream_t s) {
    VS_REQUIRE(sy.hook && sy.scratch && sy.world >= 1, "bn_bwd: bad cross-rank statistics hook");
    hipLaunchKernelGGL(bn_sync_pack_kernel, dim3(cdiv(c, 256)), dim3(256), 0, s, dbeta, dgamma, sy.scratch, c);
    VS_LAUNCH_CHECK();
    const int rc = sy.hook(sy.user, sy.scratch, 2 * (int64_t)c, 1, (void*)s);
    VS_REQUIRE(rc == 0, "bn_bwd: the cross-rank statistics hook failed (%d)", rc);
    return VS_OK;
}

// BN backward whose reduction already happened in the producing dgrad's epilogue: `g` is the masked gradient, `partial` holds
// nparts rows of per-channel (sum g, sum g * xhat).  Finalise (fp64, fixed order) and apply.
int launch_bn_bwd_from_partials(int dtype, const void* g, const void* x, const float* mean, const float* invstd, const float* gamma,
                                void* dx, void* dres, float* dgamma, float* dbeta, int64_t rows, int c, const float* partial,
                                int nparts, hipStream_t s, const BnSync* sync) {
    if (const int rc = bn_channels_ok(c, "bn_bwd")) return rc;
    RowMap m = make_rowmap(rows, c);
    // the masked gradient's apply sweep (no mask, no y, no beta) with (dgamma, dbeta) from sg / sb
    auto apply = [&](const float* sg, const float* sb, int64_t stat_rows) {
        VS_FOR_T(dtype, return launch_sweep(bn_bwd_apply<T, false, false, false>, m, 0, s, g, nullptr, x, mean, invstd, gamma, nullptr, const_cast<float*>(sg), const_cast<float*>(sb), 0, dx, dres,
                                            rows, c, m, nullptr, 0, stat_rows));
    };
    if (!sync && nparts <= vs_option("bn_inline_rows") && c <= 512 && 256 % ((2 * c) / 4) == 0) {   // few rows: finalise inside the apply sweep
        const bool pf = bn_bwd_prefetch(m);
        VS_FOR_T(dtype, return launch_sweep(pf ? bn_bwd_apply<T, false, true, true> : bn_bwd_apply<T, false, true, false>, m, 0, s, g, nullptr, x, mean, invstd,
                                            gamma, nullptr, dgamma, dbeta, 0, dx, dres, rows, c, m, partial, nparts, 0));
    }
    hipLaunchKernelGGL(bn_bwd_finalize, dim3(c), dim3(256), 0, s, partial, nparts, c, dgamma, dbeta);
    VS_LAUNCH_CHECK();
    if (!sync) return apply(dgamma, dbeta, 0);
    // sum the two vectors over the ranks, apply with the global sums and row count
    if (const int rc = bn_sync_sums(*sync, dgamma, dbeta, c, s)) return rc;
    return apply(sync->scratch + c, sync->scratch, rows * sync->world);
}

extern "C" size_t vs_bn_workspace(int64_t rows, int c) {
    (void)rows;
    return (size_t)kMaxBlocks * 2 * c * sizeof(float);
}

extern "C" int vs_bn_stats(int dtype, const void* x, int64_t rows, int c, float eps, float momentum, float* mean,
                           float* invstd, float* running_mean, float* running_var, float* workspace,
                           size_t workspace_bytes, void* stream) {
    if (const int rc = bn_channels_ok(c, "bn_stats")) return rc;
    VS_REQUIRE(workspace && workspace_bytes >= vs_bn_workspace(rows, c), "bn_stats: workspace too small");
    VS_FOR_T(dtype, return stats_t<T>(x, rows, c, eps, momentum, mean, invstd, running_mean, running_var, workspace, (hipStream_t)stream));
}

extern "C" int vs_bn_apply(int dtype, const void* x, const float* mean, const float* invstd, const float* gamma,
                           const float* beta, const void* residual, int relu, void* y, int64_t rows, int c,
                           void* stream) {
    if (const int rc = bn_channels_ok(c, "bn_apply")) return rc;
    RowMap m = make_rowmap(rows, c);
    VS_FOR_T(dtype, return launch_sweep(bn_apply_kernel<T>, m, 0, (hipStream_t)stream, x, mean, invstd, gamma, beta, residual, relu, y, rows, c, m));
}

extern "C" int vs_bn_bwd(int dtype, const void* dy, const void* y, const void* x, const float* mean,
                         const float* invstd, const float* gamma, int relu, void* dx, void* dres, float* dgamma,
                         float* dbeta, int64_t rows, int c, float* workspace, size_t workspace_bytes, void* stream) {
    VS_REQUIRE(!relu || y, "bn_bwd: the ReLU mask needs the activation y (or use vs_bn_bwd_recompute with beta)");
    return vs_bn_bwd_recompute(dtype, dy, y, x, mean, invstd, gamma, nullptr, relu, dx, dres, dgamma, dbeta, rows, c,
                               workspace, workspace_bytes, stream);
}

extern "C" int vs_bn_bwd_recompute(int dtype, const void* dy, const void* y, const void* x, const float* mean,
                                   const float* invstd, const float* gamma, const float* beta, int relu, void* dx,
                                   void* dres, float* dgamma, float* dbeta, int64_t rows, int c, float* workspace,
                                   size_t workspace_bytes, void* stream) {
    return bn_bwd_dispatch(dtype, dy, y, x, mean, invstd, gamma, beta, relu, dx, dres, dgamma, dbeta, rows, c, workspace, workspace_bytes,
                           (hipStream_t)stream);
}

// the two-sweep backward: partial sums (with the mask), finalise, apply.  (A one-launch form with a grid barrier between the two sweeps
// was built once and measured slower: 5.47 vs 4.94 ms per step.)
int bn_bwd_dispatch(int dtype, const void* dy, const void* y, const void* x, const float* mean, const float* invstd, const float* gamma,
                    const float* beta, int relu, void* dx, void* dres, float* dgamma, float* dbeta, int64_t rows, int c, float* workspace,
                    size_t workspace_bytes, hipStream_t s, const BnSync* sync) {
    if (const int rc = bn_channels_ok(c, "bn_bwd")) return rc;
    VS_REQUIRE(!relu || y || beta, "bn_bwd: need y or beta for the ReLU mask");
    VS_REQUIRE(workspace && workspace_bytes >= vs_bn_workspace(rows, c), "bn_bwd: workspace too small");
    RowMap m = make_rowmap(rows, c);
    const bool rc = relu && !y;
    VS_FOR_T(dtype, if (const int e = launch_sweep(rc ? bn_bwd_partial<T, true> : bn_bwd_partial<T, false>, m, 0, s, dy, y, x, mean, invstd, gamma, beta, relu,
                                                   rows, c, m, workspace)) return e);
    hipLaunchKernelGGL(bn_bwd_finalize, dim3(c), dim3(256), 0, s, workspace, m.nblocks, c, dgamma, dbeta);
    VS_LAUNCH_CHECK();
    const float* sum_g = dgamma; const float* sum_b = dbeta;      // the sums the apply sweep reads (cross-rank: the summed copies)
    if (sync) {
        if (const int rcs = bn_sync_sums(*sync, dgamma, dbeta, c, s)) return rcs;
        sum_g = sync->scratch + c; sum_b = sync->scratch;
    }
    VS_FOR_T(dtype, return launch_sweep(rc ? bn_bwd_apply<T, true, false, false> : bn_bwd_apply<T, false, false, false>, m, 0, s, dy, y, x, mean, invstd, gamma,
                                        beta, const_cast<float*>(sum_g), const_cast<float*>(sum_b), relu, dx, dres, rows, c, m, nullptr, 0, sync ? rows * sync->world : 0));
}

extern "C" int vs_bn_fold(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                          float eps, float* scale, float* shift, int c, void* stream) {
    hipLaunchKernelGGL(bn_fold_kernel, dim3(cdiv(c, 64)), dim3(64), 0, (hipStream_t)stream, gamma, beta, running_mean,
                       running_var, eps, scale, shift, c);
    VS_LAUNCH_CHECK();
    return VS_OK;
}

// ---- test seams: the inline sweeps and the partial-row finalise on rows the caller wrote (no kernel or launch function of their own;
// the network's plan reaches the same launch functions with the rows its convolution epilogues left)
extern "C" int vs_bn_apply_from_partials(int dtype, const void* x, const float* partial, int nparts, float eps, float momentum, float* mean,
                                         float* invstd, float* running_mean, float* running_var, const float* gamma, const float* beta,
                                         const void* residual, int relu, void* y, int64_t rows, int c, void* stream) {
    VS_REQUIRE(x && partial && mean && invstd && gamma && beta && y, "bn_apply_from_partials: null pointer");
    VS_REQUIRE(nparts >= 1 && rows >= 1 && (running_mean == nullptr) == (running_var == nullptr), "bn_apply_from_partials: bad row counts or running statistics");
    return launch_bn_apply_from_partials(dtype, x, partial, nparts, eps, momentum, mean, invstd, running_mean, running_var, gamma, beta, residual,
                                         relu, y, rows, c, (hipStream_t)stream);
}

extern "C" int vs_bn_apply_from_bins(int dtype, const void* x, const void* bins, int nb, float eps, float momentum, float* mean, float* invstd,
                                     float* running_mean, float* running_var, const float* gamma, const float* beta, const void* residual,
                                     int relu, void* y, int64_t rows, int c, int64_t stat_rows, void* stream) {
    VS_REQUIRE(x && bins && mean && invstd && gamma && beta && y, "bn_apply_from_bins: null pointer");
    VS_REQUIRE(nb >= 1 && rows >= 1 && stat_rows >= 0 && (running_mean == nullptr) == (running_var == nullptr), "bn_apply_from_bins: bad row counts or running statistics");
    return launch_bn_apply_from_bins(dtype, x, (const unsigned long long*)bins, nb, eps, momentum, mean, invstd, running_mean, running_var, gamma,
                                     beta, residual, relu, y, rows, c, (hipStream_t)stream, stat_rows);
}

extern "C" int vs_bn_bwd_from_partials(int dtype, const void* g, const void* x, const float* mean, const float* invstd, const float* gamma,
                                       void* dx, void* dres, float* dgamma, float* dbeta, int64_t rows, int c, const float* partial,
                                       int nparts, void* stream) {
    VS_REQUIRE(g && x && mean && invstd && gamma && dx && dgamma && dbeta && partial, "bn_bwd_from_partials: null pointer");
    VS_REQUIRE(nparts >= 1 && rows >= 1, "bn_bwd_from_partials: bad row counts");
    return launch_bn_bwd_from_partials(dtype, g, x, mean, invstd, gamma, dx, dres, dgamma, dbeta, rows, c, partial, nparts, (hipStream_t)stream,
                                       nullptr);
}

extern "C" int vs_bn_finalize_partials(const float* partial, int nparts, int c, int64_t rows, float eps, float momentum, float* mean,
                                       float* invstd, float* running_mean, float* running_var, void* stream) {
    VS_REQUIRE(partial && mean && invstd, "bn_finalize_partials: null pointer");
    VS_REQUIRE(nparts >= 1 && c >= 1 && rows >= 1 && (running_mean == nullptr) == (running_var == nullptr), "bn_finalize_partials: bad counts or running statistics");
    return launch_bn_finalize_partials(partial, nparts, c, rows, eps, momentum, mean, invstd, running_mean, running_var, (hipStream_t)stream);
}
