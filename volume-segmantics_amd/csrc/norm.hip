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

// ---- forward statistics ------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void bn_stats_partial(const T* __restrict__ x, int64_t rows, int c, RowMap m,
                                                      float* __restrict__ partial) {
    __shared__ float red[2][256][kVec + 1];
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
#pragma unroll
    for (int k = 0; k < kVec; ++k) { red[0][tid][k] = s[k]; red[1][tid][k] = q[k]; }
    __syncthreads();
    // thread t < C (per 8-channel group: first cv*8 threads) sums over row lanes
    for (int ch = tid; ch < m.cv * kVec; ch += 256) {
        const int g = ch / kVec, k = ch % kVec;
        float a = 0.f, b = 0.f;
        for (int j = 0; j < m.rpb; ++j) { a += red[0][j * m.cv + g][k]; b += red[1][j * m.cv + g][k]; }
        partial[((size_t)blockIdx.x * 2 + 0) * c + ch] = a;
        partial[((size_t)blockIdx.x * 2 + 1) * c + ch] = b;
    }
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
    const double dm = s / (double)rows;  // mean of (x - K)
    double var = q / (double)rows - dm * dm;
    if (var < 0.0) var = 0.0;
    const double mu = dm + (x ? (double)Elem<T>::ld(x + ch) : 0.0);
    mean[ch] = (float)mu;
    invstd[ch] = (float)(1.0 / sqrt(var + (double)eps));
    if (running_mean) {
        const double unbiased = rows > 1 ? var * (double)rows / (double)(rows - 1) : var;
        running_mean[ch] = (float)((1.0 - momentum) * (double)running_mean[ch] + momentum * mu);
        running_var[ch] = (float)((1.0 - momentum) * (double)running_var[ch] + momentum * unbiased);
    }
}

// ---- forward apply -----------------------------------------------------------------------------
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
    // kU rows per trip with every load issued before the first use: one 16-byte load in flight per thread left these sweeps
    // latency-bound at ~2.5 TB/s (a trip per ~1 us memory round trip)
    for (int64_t rb = r0 + rl; rb < r1; rb += (int64_t)kU * m.rpb) {
        float v[kU][kVec], rv[kU][kVec];
        size_t o[kU];
        bool ok[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const int64_t r = rb + (int64_t)u * m.rpb;
            ok[u] = r < r1;
            o[u] = (size_t)(ok[u] ? r : rb) * c + cvi * kVec;
            ld8(x + o[u], v[u]);
        }
        if (res) {
#pragma unroll
            for (int u = 0; u < kU; ++u) ld8(res + o[u], rv[u]);
        }
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
}

// Same, with the statistics finalised INSIDE the kernel: when the producing convolution left only a few partial rows
// (<= 64: the 16x16 / 8x8-pixel layers), every workgroup sums them itself (fp64, rows in order) instead of waiting for a
// separate finalise launch - ~1.5 us of redundant work per workgroup against ~7 us of launch + drain on the critical path.
// Workgroup 0 also publishes mean / invstd for the backward pass and updates the running statistics.
// FIXED: `partial` holds nparts rows of 64-bit fixed-point bins ([row][2][c]: sum x * 2^24, sum x^2 * 2^16, accumulated by atomic adds
// in the producing convolution's epilogue - ConvParams::stats_bins) instead of fp32 partial rows
// PF: the first trip's rows (x, residual) and gamma / beta are loaded BEFORE the statistics prologue (see Raw8 above); PF = false is
// the reference form of tests/test_hip_bn_prefetch.py and the other arm of the A/B (option bn_prefetch)
template <typename T, bool FIXED = false, bool PF = false>
__global__ __launch_bounds__(256) void bn_apply_inline_kernel(const T* __restrict__ x, const float* __restrict__ partial, int nparts,
                                                            float eps, float momentum, float* __restrict__ mean,
                                                            float* __restrict__ invstd, float* __restrict__ running_mean,
                                                            float* __restrict__ running_var, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, const T* __restrict__ res, int relu,
                                                            T* __restrict__ y, int64_t rows, int c, RowMap m, int64_t stat_rows = 0) {
    extern __shared__ float s_stat[];   // [2][c]: mean, invstd
    const int tid = threadIdx.x;
    Raw8<T> px[PF ? kU : 1], pr[PF ? kU : 1];
    float pg[PF ? kVec : 1], pb[PF ? kVec : 1];
    if constexpr (PF) {
        const int cvi = tid % m.cv, rl = tid / m.cv;
        const int64_t r0 = (int64_t)blockIdx.x * m.rows_per_block;
        const int64_t r1 = min(rows, r0 + m.rows_per_block);
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
        const double mu = s / (double)stat_rows;
        double var = q / (double)stat_rows - mu * mu;
        if (var < 0.0) var = 0.0;
        const float is = (float)(1.0 / sqrt(var + (double)eps));
        s_stat[ch] = (float)mu;
        s_stat[c + ch] = is;
        if (blockIdx.x == 0) {
            mean[ch] = (float)mu;
            invstd[ch] = is;
            if (running_mean) {
                const double unbiased = stat_rows > 1 ? var * (double)stat_rows / (double)(stat_rows - 1) : var;
                running_mean[ch] = (float)((1.0 - momentum) * (double)running_mean[ch] + momentum * mu);
                running_var[ch] = (float)((1.0 - momentum) * (double)running_var[ch] + momentum * unbiased);
            }
        }
    };
    const int cols = (2 * c) / 4;
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
    } else if (c <= 512 && 256 % cols == 0) {
        // all 256 threads: thread (column of four statistics, row group) sums its rows with 16-byte loads, four in flight;
        // the row groups meet in LDS in a fixed order (fp64 throughout: every workgroup forms the same numbers)
        __shared__ double dsum[4096];                                  // [RG][2 c]
        const int RG = 256 / cols, col = tid % cols, rg = tid / cols;
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        for (int r = rg; r < nparts; r += 4 * RG) {
            float4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if constexpr (PF) v[u] = partial_row4(partial, r + u * RG, r, nparts, 2 * c, col);
                else v[u] = (r + u * RG < nparts) ? *reinterpret_cast<const float4*>(partial + (size_t)(r + u * RG) * 2 * c + col * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) { a0 += (double)v[u].x; a1 += (double)v[u].y; a2 += (double)v[u].z; a3 += (double)v[u].w; }
        }
        double* d = dsum + (size_t)rg * 2 * c + col * 4;
        d[0] = a0; d[1] = a1; d[2] = a2; d[3] = a3;
        __syncthreads();
        for (int ch = tid; ch < c; ch += 256) {
            double s = 0.0, q = 0.0;
            for (int g2 = 0; g2 < RG; ++g2) { s += dsum[(size_t)g2 * 2 * c + ch]; q += dsum[(size_t)g2 * 2 * c + c + ch]; }
            finish(ch, s, q);
        }
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
    const int cvi = tid % m.cv, rl = tid / m.cv;
    if (rl >= m.rpb) return;
    if constexpr (PF) {
        const int64_t r0 = (int64_t)blockIdx.x * m.rows_per_block;
        const int64_t r1 = min(rows, r0 + m.rows_per_block);
        float a[kVec], b[kVec], mu[kVec];
#pragma unroll
        for (int k = 0; k < kVec; ++k) {
            const int ch = cvi * kVec + k;
            a[k] = s_stat[c + ch] * pg[k];
            b[k] = pb[k];
            mu[k] = s_stat[ch];
        }
        auto finish_trip = [&](float (&v)[kU][kVec], const float (&rv)[kU][kVec], const size_t (&o)[kU], const bool (&ok)[kU]) {
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
        };
        int64_t rb = r0 + rl;
        {      // trip 0 from the prefetched registers
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
            finish_trip(v, rv, o, ok);
            rb += (int64_t)kU * m.rpb;
        }
        // kU rows per trip with every load issued before the first use: one 16-byte load in flight per thread left these sweeps
        // latency-bound at ~2.5 TB/s (a trip per ~1 us memory round trip)
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
            finish_trip(v, rv, o, ok);
        }
    } else {     // the form without the prefetch, as it always was
        float a[kVec], b[kVec], mu[kVec];
#pragma unroll
        for (int k = 0; k < kVec; ++k) {
            const int ch = cvi * kVec + k;
            a[k] = s_stat[c + ch] * gamma[ch];
            b[k] = beta[ch];
            mu[k] = s_stat[ch];
        }
        const int64_t r0 = (int64_t)blockIdx.x * m.rows_per_block;
        const int64_t r1 = min(rows, r0 + m.rows_per_block);
        // kU rows per trip with every load issued before the first use: one 16-byte load in flight per thread left these sweeps
        // latency-bound at ~2.5 TB/s (a trip per ~1 us memory round trip)
        for (int64_t rb = r0 + rl; rb < r1; rb += (int64_t)kU * m.rpb) {
            float v[kU][kVec], rv[kU][kVec];
            size_t o[kU];
            bool ok[kU];
#pragma unroll
            for (int u = 0; u < kU; ++u) {
                const int64_t r = rb + (int64_t)u * m.rpb;
                ok[u] = r < r1;
                o[u] = (size_t)(ok[u] ? r : rb) * c + cvi * kVec;
                ld8(x + o[u], v[u]);
            }
            if (res) {
#pragma unroll
                for (int u = 0; u < kU; ++u) ld8(res + o[u], rv[u]);
            }
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
    }
}

// ---- backward ----------------------------------------------------------------------------------
// relu mask: from the stored activation y when given, otherwise recomputed as (x - mean) * invstd * gamma + beta > 0
// (bit-identical to the forward's expression; only valid for units without a residual input)
template <typename T, bool RECOMPUTE>
__global__ __launch_bounds__(256) void bn_bwd_partial(const T* __restrict__ dy, const T* __restrict__ y,
                                                    const T* __restrict__ x, const float* __restrict__ mean,
                                                    const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                    const float* __restrict__ beta, int relu, int64_t rows, int c,
                                                    RowMap m, float* __restrict__ partial) {
    __shared__ float red[2][256][kVec + 1];
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
                if (relu) {
                    if constexpr (!RECOMPUTE) {
#pragma unroll
                        for (int k = 0; k < kVec; ++k) g[u][k] = yv[u][k] > 0.f ? g[u][k] : 0.f;
                    } else {
#pragma unroll
                        for (int k = 0; k < kVec; ++k) g[u][k] = ((xv[u][k] - mu[k]) * ga[k] + be[k]) > 0.f ? g[u][k] : 0.f;
                    }
                }
#pragma unroll
                for (int k = 0; k < kVec; ++k) { s[k] += g[u][k]; q[k] += g[u][k] * (xv[u][k] - mu[k]) * is[k]; }
            }
        }
    }
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

__global__ __launch_bounds__(256) void bn_bwd_finalize(const float* __restrict__ partial, int nblocks, int c,
                                                       float* dgamma, float* dbeta) {
    const int ch = blockIdx.x;
    double s = 0.0, q = 0.0;
    strided_sum2_f64(partial, nblocks, c, ch, s, q);
    block_sum2_f64(s, q);
    if (threadIdx.x == 0) { dbeta[ch] = (float)s; dgamma[ch] = (float)q; }
}

// INLINE: the reduction's partial rows (few: <= 64) are summed by every workgroup itself (fp64, fixed order - the numbers
// bn_bwd_finalize forms); workgroup 0 publishes dgamma / dbeta.  One launch and one dependent phase fewer per unit.
// BINS (with INLINE): `partial` holds nparts rows of 64-bit fixed-point bins ([row][2][c], sums scaled by kBwdStatScale, added
// atomically by the dgrad epilogue that completed the gradient - ConvParams::bstats_bins): integer sums, any order, same bits.
// (BINS = true is instantiated by no launch in this library and run by no test: no dgrad epilogue fills such bins today.)
// PF: the first trip's rows (dy, x, y) and mean / invstd / gamma / beta are loaded before the prologue (INLINE: the partial-row or bin
// sum; otherwise the dbeta / dgamma loads and their products), and the `relu` test sits outside the row loop
template <typename T, bool RECOMPUTE, bool INLINE = false, bool BINS = false, bool PF = false>
__global__ __launch_bounds__(256) void bn_bwd_apply(const T* __restrict__ dy, const T* __restrict__ y,
                                                  const T* __restrict__ x, const float* __restrict__ mean,
                                                  const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                  const float* __restrict__ beta, float* __restrict__ dgamma,
                                                  float* __restrict__ dbeta, int relu, T* __restrict__ dx,
                                                  T* __restrict__ dres, int64_t rows, int c, RowMap m,
                                                  const float* __restrict__ partial = nullptr, int nparts = 0, int64_t stat_rows = 0) {
    const int tid = threadIdx.x;
    constexpr int NY = RECOMPUTE ? 1 : kU;
    Raw8<T> pdy[PF ? kU : 1], px[PF ? kU : 1], py[PF ? NY : 1];
    float pmu[PF ? kVec : 1], pis[PF ? kVec : 1], pga[PF ? kVec : 1], pbe[PF && RECOMPUTE ? kVec : 1];
    if constexpr (PF) {
        const int cvi = tid % m.cv, rl = tid / m.cv;
        const int64_t r0 = (int64_t)blockIdx.x * m.rows_per_block;
        const int64_t r1 = min(rows, r0 + m.rows_per_block);
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
    __shared__ float s_coef[INLINE ? 2 * 512 : 1];
    if constexpr (INLINE && BINS) {
        __shared__ long long isum[256];
        const long long* bins = reinterpret_cast<const long long*>(partial);
        const int nv = 2 * c;                                          // values per bin row: [dbeta sums | dgamma sums]
        if (nv <= 256) {
            const int RG = 256 / nv, col = tid % nv, rg = tid / nv;
            long long acc = 0;
            if (rg < RG) {
#pragma unroll 8
                for (int r = rg; r < nparts; r += RG) acc += bins[(size_t)r * nv + col];
                isum[rg * nv + col] = acc;
            }
            __syncthreads();
            for (int ch = tid; ch < nv; ch += 256) {
                long long t = 0;
                for (int g2 = 0; g2 < RG; ++g2) t += isum[g2 * nv + ch];
                const float f = (float)((double)t * (1.0 / kBwdStatScale));
                s_coef[ch] = f;
                if (blockIdx.x == 0) { if (ch < c) dbeta[ch] = f; else dgamma[ch - c] = f; }
            }
        } else {
            for (int ch = tid; ch < nv; ch += 256) {
                long long t = 0;
#pragma unroll 8
                for (int r = 0; r < nparts; ++r) t += bins[(size_t)r * nv + ch];
                const float f = (float)((double)t * (1.0 / kBwdStatScale));
                s_coef[ch] = f;
                if (blockIdx.x == 0) { if (ch < c) dbeta[ch] = f; else dgamma[ch - c] = f; }
            }
        }
        __syncthreads();
    } else if constexpr (INLINE) {
        __shared__ double dsum[INLINE ? 4096 : 1];                     // [RG][2 c]
        const int cols = (2 * c) / 4, RG = 256 / cols, col = tid % cols, rg = tid / cols;
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        for (int r = rg; r < nparts; r += 4 * RG) {
            float4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if constexpr (PF) v[u] = partial_row4(partial, r + u * RG, r, nparts, 2 * c, col);
                else v[u] = (r + u * RG < nparts) ? *reinterpret_cast<const float4*>(partial + (size_t)(r + u * RG) * 2 * c + col * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) { a0 += (double)v[u].x; a1 += (double)v[u].y; a2 += (double)v[u].z; a3 += (double)v[u].w; }
        }
        double* d = dsum + (size_t)rg * 2 * c + col * 4;
        d[0] = a0; d[1] = a1; d[2] = a2; d[3] = a3;
        __syncthreads();
        for (int ch = tid; ch < 2 * c; ch += 256) {
            double t = 0.0;
            for (int g2 = 0; g2 < RG; ++g2) t += dsum[(size_t)g2 * 2 * c + ch];
            s_coef[ch] = (float)t;                                     // [0, c): dbeta, [c, 2 c): dgamma
            if (blockIdx.x == 0) { if (ch < c) dbeta[ch] = (float)t; else dgamma[ch - c] = (float)t; }
        }
        __syncthreads();
    }
    const int cvi = tid % m.cv, rl = tid / m.cv;
    if (rl >= m.rpb) return;
    const float inv_m = 1.0f / (float)(stat_rows > 0 ? stat_rows : rows);   // (stat_rows: the sums cover the rows of every rank)
    if constexpr (PF) {
        const int64_t r0 = (int64_t)blockIdx.x * m.rows_per_block;
        const int64_t r1 = min(rows, r0 + m.rows_per_block);
        float mu[kVec], is[kVec], gi[kVec], db[kVec], dg[kVec], be[RECOMPUTE ? kVec : 1], ga[RECOMPUTE ? kVec : 1];
#pragma unroll
        for (int k = 0; k < kVec; ++k) {
            const int ch = cvi * kVec + k;
            mu[k] = pmu[k]; is[k] = pis[k]; gi[k] = pga[k] * pis[k];
            if constexpr (INLINE) { db[k] = s_coef[ch] * inv_m; dg[k] = s_coef[c + ch] * inv_m; }
            else { db[k] = dbeta[ch] * inv_m; dg[k] = dgamma[ch] * inv_m; }
            if constexpr (RECOMPUTE) { be[k] = pbe[k]; ga[k] = pis[k] * pga[k]; }
        }
        // the sweep in two versions, with and without the ReLU mask: a `relu` test inside the unrolled row loop makes hipcc branch
        // around every y load and wait for each one (four dependent rounds per trip instead of one)
        auto sweep = [&](auto relu_c) {
            constexpr bool RELU = decltype(relu_c)::value;
            auto finish_trip = [&](float (&g)[kU][kVec], const float (&xv)[kU][kVec], const float (&yv)[NY][kVec], const size_t (&o)[kU], const bool (&ok)[kU]) {
#pragma unroll
                for (int u = 0; u < kU; ++u) {
                    if (!ok[u]) continue;
                    if constexpr (RELU && !RECOMPUTE) {
#pragma unroll
                        for (int k = 0; k < kVec; ++k) g[u][k] = yv[u][k] > 0.f ? g[u][k] : 0.f;
                    } else if constexpr (RELU) {
#pragma unroll
                        for (int k = 0; k < kVec; ++k) g[u][k] = ((xv[u][k] - mu[k]) * ga[k] + be[k]) > 0.f ? g[u][k] : 0.f;
                    }
                    if (dres) st8(dres + o[u], g[u]);
                    float o8[kVec];
#pragma unroll
                    for (int k = 0; k < kVec; ++k) o8[k] = gi[k] * (g[u][k] - db[k] - (xv[u][k] - mu[k]) * is[k] * dg[k]);
                    st8(dx + o[u], o8);
                }
            };
            int64_t rb = r0 + rl;
            {      // trip 0 from the prefetched registers
                float g[kU][kVec], xv[kU][kVec], yv[NY][kVec];
                size_t o[kU];
                bool ok[kU];
                trip_offsets(rb, r1, rb < r1, m.rpb, c, cvi, o, ok);
#pragma unroll
                for (int u = 0; u < kU; ++u) {
                    unpack8(pdy[u], g[u]);
                    unpack8(px[u], xv[u]);
                    if constexpr (RELU && !RECOMPUTE) unpack8(py[u], yv[u]);
                }
                finish_trip(g, xv, yv, o, ok);
                rb += (int64_t)kU * m.rpb;
            }
            for (; rb < r1; rb += (int64_t)kU * m.rpb) {
                float g[kU][kVec], xv[kU][kVec], yv[NY][kVec];
                size_t o[kU];
                bool ok[kU];
                trip_offsets(rb, r1, true, m.rpb, c, cvi, o, ok);
#pragma unroll
                for (int u = 0; u < kU; ++u) {
                    ld8(dy + o[u], g[u]);
                    ld8(x + o[u], xv[u]);
                    if constexpr (RELU && !RECOMPUTE) ld8(y + o[u], yv[u]);
                }
                finish_trip(g, xv, yv, o, ok);
            }
        };
        if (relu) sweep(std::true_type{});
        else sweep(std::false_type{});
    } else {     // the form without the prefetch, as it always was
        float mu[kVec], is[kVec], gi[kVec], db[kVec], dg[kVec], be[RECOMPUTE ? kVec : 1], ga[RECOMPUTE ? kVec : 1];
#pragma unroll
        for (int k = 0; k < kVec; ++k) {
            const int ch = cvi * kVec + k;
            mu[k] = mean[ch]; is[k] = invstd[ch]; gi[k] = gamma[ch] * invstd[ch];
            if constexpr (INLINE) { db[k] = s_coef[ch] * inv_m; dg[k] = s_coef[c + ch] * inv_m; }
            else { db[k] = dbeta[ch] * inv_m; dg[k] = dgamma[ch] * inv_m; }
            if constexpr (RECOMPUTE) { be[k] = beta[ch]; ga[k] = invstd[ch] * gamma[ch]; }
        }
        const int64_t r0 = (int64_t)blockIdx.x * m.rows_per_block;
        const int64_t r1 = min(rows, r0 + m.rows_per_block);
        for (int64_t rb = r0 + rl; rb < r1; rb += (int64_t)kU * m.rpb) {
            float g[kU][kVec], xv[kU][kVec], yv[RECOMPUTE ? 1 : kU][kVec];
            size_t o[kU];
            bool ok[kU];
#pragma unroll
            for (int u = 0; u < kU; ++u) {
                const int64_t r = rb + (int64_t)u * m.rpb;
                ok[u] = r < r1;
                o[u] = (size_t)(ok[u] ? r : rb) * c + cvi * kVec;
                ld8(dy + o[u], g[u]);
                ld8(x + o[u], xv[u]);
                if constexpr (!RECOMPUTE) {
                    if (relu) ld8(y + o[u], yv[u]);
                }
            }
#pragma unroll
            for (int u = 0; u < kU; ++u) {
                if (!ok[u]) continue;
                if (relu) {
                    if constexpr (!RECOMPUTE) {
#pragma unroll
                        for (int k = 0; k < kVec; ++k) g[u][k] = yv[u][k] > 0.f ? g[u][k] : 0.f;
                    } else {
#pragma unroll
                        for (int k = 0; k < kVec; ++k) g[u][k] = ((xv[u][k] - mu[k]) * ga[k] + be[k]) > 0.f ? g[u][k] : 0.f;
                    }
                }
                if (dres) st8(dres + o[u], g[u]);
                float o8[kVec];
#pragma unroll
                for (int k = 0; k < kVec; ++k) o8[k] = gi[k] * (g[u][k] - db[k] - (xv[u][k] - mu[k]) * is[k] * dg[k]);
                st8(dx + o[u], o8);
            }
        }
    }
}

__global__ void bn_fold_kernel(const float* gamma, const float* beta, const float* rm, const float* rv, float eps,
                               float* scale, float* shift, int c) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= c) return;
    const float s = gamma[i] / sqrtf(rv[i] + eps);
    scale[i] = s;
    shift[i] = beta[i] - rm[i] * s;
}

template <typename T>
int stats_t(const void* x, int64_t rows, int c, float eps, float momentum, float* mean, float* invstd, float* rm,
            float* rv, float* ws, hipStream_t s) {
    RowMap m = make_rowmap(rows, c);
    hipLaunchKernelGGL(bn_stats_partial<T>, dim3(m.nblocks), dim3(256), 0, s, (const T*)x, rows, c, m, ws);
    VS_LAUNCH_CHECK();
    hipLaunchKernelGGL(bn_stats_finalize<T>, dim3(c), dim3(256), 0, s, ws, (const T*)x, m.nblocks, c, rows, eps,
                       momentum, mean, invstd, rm, rv);
    VS_LAUNCH_CHECK();
    return VS_OK;
}

// which form of the sweeps a launch takes (read at launch time; 0 = the forms without the prefetched first trip)
bool bn_prefetch() { return vs_option("bn_prefetch") != 0; }
// The prefetch form of bn_bwd_apply holds the first trip beside the parameters: 170 registers against 128 for bf16, two workgroups
// per CU instead of four.  It takes the INLINE launches (11.7 -> 8.9 us median in the traced step) whose workgroups are all resident
// at once either way - the latency-bound deep layers.  The plain apply sweep measured no faster in that form (one hidden round,
// paid for with the occupancy) and keeps the form without it, as does bn_bwd_partial.
bool bn_bwd_prefetch(const RowMap& m) { return bn_prefetch() && m.nblocks <= 2 * device_cus(); }

}  // namespace

// train-mode BN forward from the conv epilogue's partial rows in ONE launch (nparts small): finalise + normalise
int launch_bn_apply_from_partials(int dtype, const void* x, const float* partial, int nparts, float eps, float momentum, float* mean,
                                  float* invstd, float* running_mean, float* running_var, const float* gamma, const float* beta,
                                  const void* residual, int relu, void* y, int64_t rows, int c, hipStream_t s) {
    VS_REQUIRE(c % kVec == 0 && c <= 2048, "bn_apply: unsupported channel count %d", c);
    RowMap m = make_rowmap(rows, c);
    const size_t lds = 2 * (size_t)c * sizeof(float);
#define VS_APPLY_INLINE(T, PF) hipLaunchKernelGGL((bn_apply_inline_kernel<T, false, PF>), dim3(m.nblocks), dim3(256), lds, s, (const T*)x, partial, nparts, \
                                                 eps, momentum, mean, invstd, running_mean, running_var, gamma, beta, (const T*)residual, relu, (T*)y, rows, c, m)
    VS_FOR_T(dtype, { if (bn_prefetch()) VS_APPLY_INLINE(T, true); else VS_APPLY_INLINE(T, false); });
#undef VS_APPLY_INLINE
    VS_LAUNCH_CHECK();
    return VS_OK;
}

int launch_bn_apply_from_bins(int dtype, const void* x, const unsigned long long* bins, int nb, float eps, float momentum, float* mean,
                              float* invstd, float* running_mean, float* running_var, const float* gamma, const float* beta,
                              const void* residual, int relu, void* y, int64_t rows, int c, hipStream_t s, int64_t stat_rows) {
    VS_REQUIRE(c % kVec == 0 && c <= 2048 && nb >= 1, "bn_apply: unsupported channel count %d", c);
    RowMap m = make_rowmap(rows, c);
    const size_t lds = 2 * (size_t)c * sizeof(float) + (size_t)std::max(256, 2 * c) * sizeof(long long);
#define VS_APPLY_BINS(T, PF) hipLaunchKernelGGL((bn_apply_inline_kernel<T, true, PF>), dim3(m.nblocks), dim3(256), lds, s, (const T*)x, (const float*)bins, nb, \
                                               eps, momentum, mean, invstd, running_mean, running_var, gamma, beta, (const T*)residual, relu, (T*)y, rows, c, m, stat_rows)
    VS_FOR_T(dtype, { if (bn_prefetch()) VS_APPLY_BINS(T, true); else VS_APPLY_BINS(T, false); });
#undef VS_APPLY_BINS
    VS_LAUNCH_CHECK();
    return VS_OK;
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

// BN backward whose reduction already happened in the producing dgrad's epilogue: `g` is the masked gradient, `partial` holds
// nparts rows of per-channel (sum g, sum g * xhat).  Finalise (fp64, fixed order) and apply.
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

int launch_bn_bwd_from_partials(int dtype, const void* g, const void* x, const float* mean, const float* invstd, const float* gamma,
                                void* dx, void* dres, float* dgamma, float* dbeta, int64_t rows, int c, const float* partial,
                                int nparts, hipStream_t s, const BnSync* sync) {
    VS_REQUIRE(c % kVec == 0 && c <= 2048, "bn_bwd: unsupported channel count %d", c);
    RowMap m = make_rowmap(rows, c);
    const bool pf = bn_bwd_prefetch(m);
    // the masked gradient's apply sweep: (dgamma, dbeta) from SG / SB, or (INLINE) summed from the PARTIAL rows inside the sweep
#define VS_BWD_APPLY_G(T, INLINE, PF, SG, SB, PARTIAL, NPARTS, STAT_ROWS)                                                                  \
    hipLaunchKernelGGL((bn_bwd_apply<T, false, INLINE, false, PF>), dim3(m.nblocks), dim3(256), 0, s, (const T*)g, (const T*)nullptr, (const T*)x, mean, \
                       invstd, gamma, (const float*)nullptr, SG, SB, 0, (T*)dx, (T*)dres, rows, c, m, PARTIAL, NPARTS, STAT_ROWS)
    if (sync) {      // finalise locally, sum the two vectors over the ranks, apply with the global sums and row count
        hipLaunchKernelGGL(bn_bwd_finalize, dim3(c), dim3(256), 0, s, partial, nparts, c, dgamma, dbeta);
        VS_LAUNCH_CHECK();
        if (const int rc = bn_sync_sums(*sync, dgamma, dbeta, c, s)) return rc;
        VS_FOR_T(dtype, VS_BWD_APPLY_G(T, false, false, sync->scratch + c, sync->scratch, (const float*)nullptr, 0, rows * sync->world));
        VS_LAUNCH_CHECK();
        return VS_OK;
    }
    if (nparts <= vs_option("bn_inline_rows") && c <= 512 && 256 % ((2 * c) / 4) == 0) {   // few rows: finalise inside the apply sweep
        VS_FOR_T(dtype, { if (pf) VS_BWD_APPLY_G(T, true, true, dgamma, dbeta, partial, nparts, 0);
                          else VS_BWD_APPLY_G(T, true, false, dgamma, dbeta, partial, nparts, 0); });
        VS_LAUNCH_CHECK();
        return VS_OK;
    }
    hipLaunchKernelGGL(bn_bwd_finalize, dim3(c), dim3(256), 0, s, partial, nparts, c, dgamma, dbeta);
    VS_LAUNCH_CHECK();
    VS_FOR_T(dtype, VS_BWD_APPLY_G(T, false, false, dgamma, dbeta, (const float*)nullptr, 0, 0));
    VS_LAUNCH_CHECK();
#undef VS_BWD_APPLY_G
    return VS_OK;
}

extern "C" size_t vs_bn_workspace(int64_t rows, int c) {
    (void)rows;
    return (size_t)kMaxBlocks * 2 * c * sizeof(float);
}

extern "C" int vs_bn_stats(int dtype, const void* x, int64_t rows, int c, float eps, float momentum, float* mean,
                           float* invstd, float* running_mean, float* running_var, float* workspace,
                           size_t workspace_bytes, void* stream) {
    VS_REQUIRE(c % kVec == 0 && c <= 2048,
               "bn_stats: unsupported channel count %d", c);
    VS_REQUIRE(workspace && workspace_bytes >= vs_bn_workspace(rows, c), "bn_stats: workspace too small");
    VS_FOR_T(dtype, return stats_t<T>(x, rows, c, eps, momentum, mean, invstd, running_mean, running_var, workspace, (hipStream_t)stream));
}

extern "C" int vs_bn_apply(int dtype, const void* x, const float* mean, const float* invstd, const float* gamma,
                           const float* beta, const void* residual, int relu, void* y, int64_t rows, int c,
                           void* stream) {
    VS_REQUIRE(c % kVec == 0 && c <= 2048, "bn_apply: unsupported channel count %d", c);
    RowMap m = make_rowmap(rows, c);
    hipStream_t s = (hipStream_t)stream;
    VS_FOR_T(dtype, hipLaunchKernelGGL(bn_apply_kernel<T>, dim3(m.nblocks), dim3(256), 0, s, (const T*)x, mean, invstd, gamma,
                           beta, (const T*)residual, relu, (T*)y, rows, c, m));
    VS_LAUNCH_CHECK();
    return VS_OK;
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
                           nullptr, (hipStream_t)stream);
}

// ctl: pre-zeroed, self-re-arming barrier counters (the network's plan keeps them); null = take the last 16 bytes of the
// workspace and zero them first (the stand-alone operator)
int bn_bwd_dispatch(int dtype, const void* dy, const void* y, const void* x, const float* mean, const float* invstd, const float* gamma,
                    const float* beta, int relu, void* dx, void* dres, float* dgamma, float* dbeta, int64_t rows, int c, float* workspace,
                    size_t workspace_bytes, unsigned* ctl, hipStream_t s, const BnSync* sync) {
    VS_REQUIRE(c % kVec == 0 && c <= 2048, "bn_bwd: unsupported channel count %d", c);
    VS_REQUIRE(!relu || y || beta, "bn_bwd: need y or beta for the ReLU mask");
    VS_REQUIRE(workspace && workspace_bytes >= vs_bn_workspace(rows, c), "bn_bwd: workspace too small");
    (void)ctl;      // (a one-launch form with a grid barrier between the two sweeps was built in round 3 and measured slower: 5.47 vs 4.94 ms per step)
    RowMap m = make_rowmap(rows, c);
    const bool rc = relu && !y;
#define VS_BWD_PARTIAL(T, R) hipLaunchKernelGGL((bn_bwd_partial<T, R>), dim3(m.nblocks), dim3(256), 0, s, (const T*)dy, (const T*)y, \
                                                (const T*)x, mean, invstd, gamma, beta, relu, rows, c, m, workspace)
    const float* sum_g = dgamma; const float* sum_b = dbeta;      // the sums the apply sweep reads (cross-rank: the summed copies)
    const int64_t stat_rows = sync ? rows * sync->world : 0;
#define VS_BWD_APPLY(T, R) hipLaunchKernelGGL((bn_bwd_apply<T, R>), dim3(m.nblocks), dim3(256), 0, s, (const T*)dy, (const T*)y, \
                                              (const T*)x, mean, invstd, gamma, beta, const_cast<float*>(sum_g), const_cast<float*>(sum_b), relu, \
                                              (T*)dx, (T*)dres, rows, c, m, (const float*)nullptr, 0, stat_rows)
    VS_FOR_T(dtype, { if (rc) VS_BWD_PARTIAL(T, true); else VS_BWD_PARTIAL(T, false); });
    VS_LAUNCH_CHECK();
    hipLaunchKernelGGL(bn_bwd_finalize, dim3(c), dim3(256), 0, s, workspace, m.nblocks, c, dgamma, dbeta);
    VS_LAUNCH_CHECK();
    if (sync) {
        if (const int rcs = bn_sync_sums(*sync, dgamma, dbeta, c, s)) return rcs;
        sum_g = sync->scratch + c; sum_b = sync->scratch;
    }
    VS_FOR_T(dtype, { if (rc) VS_BWD_APPLY(T, true); else VS_BWD_APPLY(T, false); });
    VS_LAUNCH_CHECK();
#undef VS_BWD_PARTIAL
#undef VS_BWD_APPLY
    return VS_OK;
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
