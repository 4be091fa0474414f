// Surface distances between two label volumes (gfx950): the surface voxels of one class, the exact squared Euclidean distance
// transform of a set of seed voxels, and the histogram of the squared distances found at the voxels of a surface.  With unit
// voxels a squared distance is an integer, so every step here is integer arithmetic and the results are the same bits on every
// run; Hausdorff distances, the average symmetric surface distance and the surface Dice follow from two such histograms on
// the host (utilities/surface_distance.py).
//
// vs_label_surface: one sweep, 16 consecutive voxels of the flat volume per lane.  Class membership of the 16 voxels and of
// their six neighbour vectors (the same 16 positions one row / one plane away, read as unaligned 16-byte vectors; the x
// neighbours are the vector itself shifted by one voxel, plus one byte at each end) is held as 16-bit masks, the volume's faces
// as masks of the coordinates, and the surface is `member & ~(interior along x & along y & along z)`.  A vector without a
// member costs its own load and one store.
//
// vs_edt_squared: separable, three launches, lanes along x in each.
//  * x: one wave per row.  A forward max-scan of "index of the last seed at or before x" (wave scan per 64 voxels, carried
//    from one 64 to the next), then the mirrored backward min-scan; d2 = min(x - left, right - x)^2, 0xFFFFFFFF in a row
//    without a seed.
//  * y, z: out(p) = min over p' of f(p') + (p - p')^2 down a column.  A workgroup owns 64 neighbouring columns over the WHOLE
//    axis: it stages them in LDS (rows of 64 dwords, so loads, stores and LDS accesses are all lane-contiguous), and every
//    lane searches outwards from p: best = f(p); for k = 1, 2, ... while k^2 < best: best = min(best, f(p -+ k) + k^2).  No
//    candidate at offset k with k^2 >= best can improve, so stopping there is exact; the cost is the answer's distance, the
//    axis length at worst.  The staged tile makes the pass in place.  An axis longer than kMaxLdsAxis does not fit the tile:
//    the same search then reads global memory, from one buffer into another (that is what the workspace is for).
//  No workgroup waits for another; every loop is bounded by an axis length.
//
// vs_edt_squared_scaled: the same three launches on a grid whose steps along z, y, x are the integers wz, wy, wx: the squared
// distance is qz dz^2 + qy dy^2 + qx dx^2, q = w^2, still an integer.  The x pass writes qx m^2, the column passes search with
// kk = q k^2 and keep the stop rule kk >= best, so a coarse axis ends its search after fewer steps.  The kernels are the same
// templates; the unscaled instantiations never read the weight.
//
// vs_surface_distance_histogram: on a good prediction most surface voxels sit at d2 = 0, so bins 0..2 are counted in registers
// and the next bins in an LDS histogram; a workgroup issues one 64-bit global atomic per non-zero small bin, and only the
// far bins (rare, spread) go to global atomics one by one.
#include "common.h"
#include "prof.h"

namespace {

constexpr uint32_t kInf = 0xFFFFFFFFu;
constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kAxisThreads = 512, kAxisWaves = kAxisThreads / 64;
constexpr int kTileCols = 64;                  // columns of one LDS tile: one wave's width
constexpr int kMaxLdsAxis = 512;               // longest axis a tile holds: 512 * 64 * 4 B = 128 KiB of the CU's 160 KiB
constexpr int kSmallBins = 1024;               // bins of the workgroup's LDS histogram
constexpr int kRegBins = 3;                    // bins counted in registers

// (Z-1)^2 + (Y-1)^2 + (X-1)^2 < 2^32 - 1: every squared distance in the volume is a uint32 below the "no seed" mark
bool extents_fit(int64_t Z, int64_t Y, int64_t X) {
    if (Z < 1 || Y < 1 || X < 1 || Z > 65536 || Y > 65536 || X > 65536) return false;
    const uint64_t s = (uint64_t)((Z - 1) * (Z - 1)) + (uint64_t)((Y - 1) * (Y - 1)) + (uint64_t)((X - 1) * (X - 1));
    return s < 0xFFFFFFFFull;
}

// ---- surface -------------------------------------------------------------------------------------------------------------------
// bytes [i, i + 16) of p; positions outside [0, n) read as 0 (their membership bits are never used: the face masks cover them)
__device__ __forceinline__ uint4 load16(const uint8_t* __restrict__ p, int64_t i, int64_t n) {
    uint4 r;
    if (i >= 0 && i + 16 <= n) {
        __builtin_memcpy(&r, p + i, 16);
        return r;
    }
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int64_t k = i + j;
        if (k >= 0 && k < n) w[j >> 2] |= (uint32_t)p[k] << (8 * (j & 3));
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// bit j = voxel j of the vector belongs to the class
__device__ __forceinline__ uint32_t members16(const uint8_t* member, const uint4 v) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) m |= (uint32_t)member[(w[j >> 2] >> (8 * (j & 3))) & 0xff] << j;
    return m;
}

__device__ __forceinline__ uint32_t spread4(uint32_t bits) {     // 4 mask bits -> 4 bytes of 0 / 1
    return (bits & 1u) | ((bits & 2u) << 7) | ((bits & 4u) << 14) | ((bits & 8u) << 21);
}

__global__ __launch_bounds__(kThreads) void surface_kernel(const uint8_t* __restrict__ labels, const uint8_t* __restrict__ lut, int cls,
                                                         int64_t Z, int64_t Y, int64_t X, int64_t n, uint8_t* __restrict__ surface,
                                                         unsigned long long* __restrict__ count) {
    __shared__ uint8_t member[256];
    __shared__ uint32_t wave_sum[kWaves];
    const int tid = threadIdx.x;
    member[tid] = (uint8_t)((lut ? (int)lut[tid] : tid) == cls);     // cls <= 253: the table's marks 254 / 255 are never members
    __syncthreads();

    const int64_t plane = Y * X, nvec = (n + 15) >> 4;
    uint32_t mine = 0;
    for (int64_t v = (int64_t)blockIdx.x * kThreads + tid; v < nvec; v += (int64_t)gridDim.x * kThreads) {
        const int64_t i0 = v << 4;
        const int len = n - i0 < 16 ? (int)(n - i0) : 16;
        const uint32_t live = len == 16 ? 0xffffu : (1u << len) - 1u;
        const uint32_t c = members16(member, load16(labels, i0, n)) & live;
        uint32_t surf = 0;
        if (c) {
            // faces of the volume as masks over the 16 voxels
            int64_t x = i0 % X, r = i0 / X;
            int64_t y = r % Y, z = r / Y;
            uint32_t fx = 0, fy = 0, fz = 0;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                fx |= (uint32_t)(x == 0 || x == X - 1) << j;
                fy |= (uint32_t)(y == 0 || y == Y - 1) << j;
                fz |= (uint32_t)(z == 0 || z == Z - 1) << j;
                if (++x == X) { x = 0; if (++y == Y) { y = 0; ++z; } }
            }
            uint32_t interior = 0xffffu;
            if (X > 1) {        // an axis of length 1 has no neighbours and is skipped
                const uint32_t before = i0 > 0 ? member[labels[i0 - 1]] : 0u;
                const uint32_t after = i0 + 16 < n ? member[labels[i0 + 16]] : 0u;
                interior &= ((c << 1) | before) & ((c >> 1) | (after << 15)) & ~fx;
            }
            if (Y > 1) interior &= members16(member, load16(labels, i0 - X, n)) & members16(member, load16(labels, i0 + X, n)) & ~fy;
            if (Z > 1) interior &= members16(member, load16(labels, i0 - plane, n)) & members16(member, load16(labels, i0 + plane, n)) & ~fz;
            surf = c & ~interior;
            mine += (uint32_t)__popc(surf);
        }
        if (len == 16) {
            *reinterpret_cast<uint4*>(surface + i0) = make_uint4(spread4(surf), spread4(surf >> 4), spread4(surf >> 8), spread4(surf >> 12));
        } else {
            for (int j = 0; j < len; ++j) surface[i0 + j] = (uint8_t)((surf >> j) & 1u);
        }
    }
    if (count) {        // uniform over the grid
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mine += __shfl_down(mine, o, 64);
        if ((tid & 63) == 0) wave_sum[tid >> 6] = mine;
        __syncthreads();
        if (tid == 0) {
            unsigned long long s = 0;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) s += wave_sum[w];
            if (s) atomicAdd(count, s);
        }
    }
}

// ---- distance transform ----------------------------------------------------------------------------------------------------------
// in-row pass: one wave per row, lanes along x.  kScaled: the squared step along x is q (vs_edt_squared_scaled), else 1.
template <bool kScaled>
__global__ __launch_bounds__(kThreads) void edt_x_kernel(const uint8_t* __restrict__ seeds, int64_t rows, int X, uint32_t* d2, uint32_t q) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int kNone = 0x7fffffff;
    for (int64_t row = (int64_t)blockIdx.x * kWaves + wave; row < rows; row += (int64_t)gridDim.x * kWaves) {   // uniform over the wave
        const uint8_t* s = seeds + row * X;
        uint32_t* d = d2 + row * X;
        int carry = -1;                                   // index of the last seed at or before x; -1: none yet
        for (int x0 = 0; x0 < X; x0 += 64) {
            const int x = x0 + lane;
            int idx = (x < X && s[x]) ? x : -1;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int t = __shfl_up(idx, o, 64);
                if (lane >= o) idx = idx > t ? idx : t;
            }
            idx = idx > carry ? idx : carry;
            carry = __shfl(idx, 63, 64);
            if (x < X) d[x] = (uint32_t)idx;              // -1 is stored as kInf
        }
        carry = kNone;                                    // index of the first seed at or after x
        for (int x0 = ((X - 1) / 64) * 64; x0 >= 0; x0 -= 64) {
            const int x = x0 + lane;
            int idx = (x < X && s[x]) ? x : kNone;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int t = __shfl_down(idx, o, 64);
                if (lane + o < 64) idx = idx < t ? idx : t;
            }
            idx = idx < carry ? idx : carry;
            carry = __shfl(idx, 0, 64);
            if (x < X) {                                  // the same lane stored d[x] above
                const uint32_t left = d[x];
                const uint32_t dl = left == kInf ? kInf : (uint32_t)x - left;
                const uint32_t dr = idx == kNone ? kInf : (uint32_t)(idx - x);
                const uint32_t m = dl < dr ? dl : dr;
                if (kScaled) d[x] = m == kInf ? kInf : q * m * m;    // q m^2 <= q (X-1)^2 < 2^32 by the bound on the extents
                else d[x] = m == kInf ? kInf : m * m;     // m <= 65535
            }
        }
    }
}

// column pass: address of (outer o, position p, column c) = (o * L + p) * inner + c.  y: outer = Z, L = Y, inner = X;
// z: outer = 1, L = Z, inner = Y * X.  kLds: src may equal dst.  kScaled: the squared step along the axis is q, else 1; the stop
// rule holds under a weight as it does without: no candidate at offset k can beat best once q k^2 >= best.
template <bool kLds, bool kScaled>
__global__ __launch_bounds__(kAxisThreads) void edt_axis_kernel(const uint32_t* src, uint32_t* dst, int64_t inner, int L, int64_t tiles_per_outer,
                                                              uint32_t q) {
    extern __shared__ __attribute__((aligned(16))) uint32_t tile[];      // [L][kTileCols] when kLds
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t outer = blockIdx.x / tiles_per_outer, t = blockIdx.x - outer * tiles_per_outer;
    const int64_t col = t * kTileCols + lane;
    const bool ok = col < inner;
    const int64_t base = outer * L * inner + (ok ? col : 0);
    const uint32_t* s = src + base;
    uint32_t* d = dst + base;
    if (kLds) {
        for (int p = wave; p < L; p += kAxisWaves) tile[p * kTileCols + lane] = ok ? s[(int64_t)p * inner] : kInf;
        __syncthreads();
    }
    if (!ok) return;
    for (int p = wave; p < L; p += kAxisWaves) {
        uint32_t best = kLds ? tile[p * kTileCols + lane] : s[(int64_t)p * inner];
        const int reach = p > L - 1 - p ? p : L - 1 - p;
        for (int k = 1; k <= reach; ++k) {               // k <= 65535: k * k fits
            // scaled: q k^2 <= q (L-1)^2 < 2^32 by the bound on the extents
            const uint32_t kk = kScaled ? q * (uint32_t)k * (uint32_t)k : (uint32_t)k * (uint32_t)k;
            if (kk >= best) break;
            if (p >= k) {
                const uint32_t f = kLds ? tile[(p - k) * kTileCols + lane] : s[(int64_t)(p - k) * inner];
                if (f != kInf && f + kk < best) best = f + kk;     // f + kk is a squared distance inside the volume: no wrap
            }
            if (p + k < L) {
                const uint32_t f = kLds ? tile[(p + k) * kTileCols + lane] : s[(int64_t)(p + k) * inner];
                if (f != kInf && f + kk < best) best = f + kk;
            }
        }
        d[(int64_t)p * inner] = best;
    }
}

// ---- histogram -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void distance_histogram_kernel(const uint8_t* __restrict__ from_surface, const uint32_t* __restrict__ d2,
                                                                    int64_t n, int64_t bins, unsigned long long* __restrict__ hist) {
    __shared__ uint32_t small[kSmallBins];
    const int tid = threadIdx.x;
    for (int i = tid; i < kSmallBins; i += kThreads) small[i] = 0;
    __syncthreads();
    uint32_t reg[kRegBins] = {0u, 0u, 0u};
    const uint64_t last = (uint64_t)bins - 1;
    auto add = [&](uint32_t v) {
        const uint64_t b = v < last ? v : last;
        if (b == 0) ++reg[0];
        else if (b == 1) ++reg[1];
        else if (b == 2) ++reg[2];
        else if (b < (uint64_t)kSmallBins) atomicAdd(&small[b], 1u);
        else atomicAdd(hist + b, 1ull);
    };
    const int64_t nq = n >> 2;
    const uint32_t* s4 = reinterpret_cast<const uint32_t*>(from_surface);
    const uint4* d4 = reinterpret_cast<const uint4*>(d2);
    for (int64_t q = (int64_t)blockIdx.x * kThreads + tid; q < nq; q += (int64_t)gridDim.x * kThreads) {
        const uint32_t s = s4[q];
        if (!s) continue;
        const uint4 d = d4[q];
        if (s & 0x000000ffu) add(d.x);
        if (s & 0x0000ff00u) add(d.y);
        if (s & 0x00ff0000u) add(d.z);
        if (s & 0xff000000u) add(d.w);
    }
    if (blockIdx.x == 0 && tid < (int)(n & 3)) {
        const int64_t i = (nq << 2) + tid;
        if (from_surface[i]) add(d2[i]);
    }
#pragma unroll
    for (int r = 0; r < kRegBins; ++r) {
        uint32_t v = reg[r];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        if ((tid & 63) == 0 && v) atomicAdd(&small[r], v);
    }
    __syncthreads();
    for (int i = tid; i < kSmallBins && i < bins; i += kThreads)
        if (small[i]) atomicAdd(hist + i, (unsigned long long)small[i]);
}

}  // namespace

extern "C" int vs_label_surface(const uint8_t* labels, const uint8_t* lut, int cls, int64_t Z, int64_t Y, int64_t X, uint8_t* surface,
                                int64_t* count, void* stream) {
    VS_REQUIRE(labels && surface, "label_surface: null volume");
    VS_REQUIRE(Z >= 1 && Y >= 1 && X >= 1 && Z < (1LL << 40) / Y && Z * Y < (1LL << 40) / X, "label_surface: bad extents %lld x %lld x %lld",
               (long long)Z, (long long)Y, (long long)X);
    VS_REQUIRE(cls >= 0 && cls <= 253, "label_surface: class %d - classes are 0..253 (254 / 255 are the table's marks)", cls);
    VS_REQUIRE(((uintptr_t)labels | (uintptr_t)surface) % 16 == 0, "label_surface: volumes must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (count) VS_CHECK_HIP(hipMemsetAsync(count, 0, sizeof(int64_t), s));
    const int64_t n = Z * Y * X, nvec = (n + 15) >> 4;
    int64_t grid = (nvec + kThreads - 1) / kThreads;      // a lane counts at most 2^40 / 16 / kThreads < 2^32 voxels
    if (grid > persistent_workgroups()) grid = persistent_workgroups();
    hipLaunchKernelGGL(surface_kernel, dim3((unsigned)grid), dim3(kThreads), 0, s, labels, lut, cls, Z, Y, X, n, surface,
                       (unsigned long long*)count);
    VS_LAUNCH_CHECK();
    return VS_OK;
}

// bytes of workspace vs_edt_squared needs: none while the y and z axes fit the LDS tile, one uint32 volume otherwise
extern "C" size_t vs_edt_workspace_bytes(int64_t Z, int64_t Y, int64_t X) {
    if (!extents_fit(Z, Y, X)) return 0;
    const bool global_y = Y > kMaxLdsAxis, global_z = Z > kMaxLdsAxis;
    return (global_y || global_z) ? (size_t)(Z * Y * X) * sizeof(uint32_t) : 0;
}

namespace {

// the three passes of both entry points; q: the squared weights of z, y, x (read only when kScaled)
template <bool kScaled>
int edt_passes(const uint8_t* seeds, int64_t Z, int64_t Y, int64_t X, const uint32_t q[3], uint32_t* d2, void* workspace, hipStream_t s) {
    const int64_t rows = Z * Y;
    const double volume = (double)(Z * Y * X);             // profile records (tools/surface_probe.py): x, then y, then z, in launch order
    {
        ProfScope prof(PK_POOL_MISC, 0.0, 5.0 * volume, s);          // seeds read, d2 written
        int64_t grid = (rows + kWaves - 1) / kWaves;
        if (grid > 4 * (int64_t)persistent_workgroups()) grid = 4 * (int64_t)persistent_workgroups();
        hipLaunchKernelGGL(edt_x_kernel<kScaled>, dim3((unsigned)grid), dim3(kThreads), 0, s, seeds, rows, (int)X, d2, q[2]);
        VS_LAUNCH_CHECK();
    }
    uint32_t* cur = d2;
    uint32_t* other = (uint32_t*)workspace;
    const struct { int64_t outer, inner; int L; uint32_t q; } passes[2] = {{Z, X, (int)Y, q[1]}, {1, Y * X, (int)Z, q[0]}};
    for (const auto& p : passes) {
        if (p.L == 1) continue;
        const int64_t tiles = (p.inner + kTileCols - 1) / kTileCols;
        VS_REQUIRE(p.outer * tiles < (1LL << 31), "edt_squared: volume too large");
        const dim3 grid((unsigned)(p.outer * tiles));
        ProfScope prof(PK_POOL_MISC, 0.0, 8.0 * volume, s);          // d2 read and written
        if (p.L <= kMaxLdsAxis) {
            const size_t lds = (size_t)p.L * kTileCols * sizeof(uint32_t);
            if (lds > 64 * 1024)
                VS_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&edt_axis_kernel<true, kScaled>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 kMaxLdsAxis * kTileCols * (int)sizeof(uint32_t)));
            hipLaunchKernelGGL((edt_axis_kernel<true, kScaled>), grid, dim3(kAxisThreads), lds, s, cur, cur, p.inner, p.L, tiles, p.q);
        } else {
            hipLaunchKernelGGL((edt_axis_kernel<false, kScaled>), grid, dim3(kAxisThreads), 0, s, cur, other, p.inner, p.L, tiles, p.q);
            uint32_t* t = cur; cur = other; other = t;
        }
        VS_LAUNCH_CHECK();
    }
    if (cur != d2) VS_CHECK_HIP(hipMemcpyAsync(d2, cur, (size_t)(Z * Y * X) * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
    return VS_OK;
}

}  // namespace

extern "C" int vs_edt_squared(const uint8_t* seeds, int64_t Z, int64_t Y, int64_t X, uint32_t* d2, void* workspace, size_t workspace_bytes,
                              void* stream) {
    VS_REQUIRE(extents_fit(Z, Y, X),
               "edt_squared: extents %lld x %lld x %lld - (Z-1)^2 + (Y-1)^2 + (X-1)^2 must be below 2^32 - 1 for squared distances to fit a uint32",
               (long long)Z, (long long)Y, (long long)X);
    VS_REQUIRE(seeds && d2, "edt_squared: null volume");
    VS_REQUIRE((uintptr_t)d2 % 4 == 0 && (uintptr_t)workspace % 4 == 0, "edt_squared: d2 and workspace must be 4-byte aligned");
    const size_t need = vs_edt_workspace_bytes(Z, Y, X);
    VS_REQUIRE(workspace_bytes >= need && (need == 0 || workspace), "edt_squared: workspace of %zu bytes, %zu needed (vs_edt_workspace_bytes)",
               workspace_bytes, need);
    const uint32_t q[3] = {1u, 1u, 1u};
    return edt_passes<false>(seeds, Z, Y, X, q, d2, workspace, (hipStream_t)stream);
}

extern "C" int vs_edt_squared_scaled(const uint8_t* seeds, int64_t Z, int64_t Y, int64_t X, int wz, int wy, int wx, uint32_t* d2, void* workspace,
                                     size_t workspace_bytes, void* stream) {
    VS_REQUIRE(weighted_distances_fit(Z, Y, X, wz, wy, wx),
               "edt_squared_scaled: extents %lld x %lld x %lld under weights %d, %d, %d - every weight must be 1..64 and wz^2 (Z-1)^2 + wy^2 (Y-1)^2 + "
               "wx^2 (X-1)^2 below 2^32 - 1 for squared distances to fit a uint32",
               (long long)Z, (long long)Y, (long long)X, wz, wy, wx);
    VS_REQUIRE(seeds && d2, "edt_squared_scaled: null volume");
    VS_REQUIRE((uintptr_t)d2 % 4 == 0 && (uintptr_t)workspace % 4 == 0, "edt_squared_scaled: d2 and workspace must be 4-byte aligned");
    const size_t need = vs_edt_workspace_bytes(Z, Y, X);       // the weighted bound is the tighter one: the extents fit here too
    VS_REQUIRE(workspace_bytes >= need && (need == 0 || workspace), "edt_squared_scaled: workspace of %zu bytes, %zu needed (vs_edt_workspace_bytes)",
               workspace_bytes, need);
    const uint32_t q[3] = {(uint32_t)(wz * wz), (uint32_t)(wy * wy), (uint32_t)(wx * wx)};
    return edt_passes<true>(seeds, Z, Y, X, q, d2, workspace, (hipStream_t)stream);
}

extern "C" int vs_surface_distance_histogram(const uint8_t* from_surface, const uint32_t* d2, int64_t n, int64_t bins, int64_t* hist,
                                             void* stream) {
    VS_REQUIRE(from_surface && d2 && hist, "surface_distance_histogram: null argument");
    VS_REQUIRE(n >= 1 && n < (1LL << 40) && bins >= 1 && bins <= (1LL << 33), "surface_distance_histogram: bad sizes n = %lld, bins = %lld",
               (long long)n, (long long)bins);
    VS_REQUIRE((uintptr_t)from_surface % 4 == 0 && (uintptr_t)d2 % 16 == 0, "surface_distance_histogram: the mask must be 4-byte, d2 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    VS_CHECK_HIP(hipMemsetAsync(hist, 0, (size_t)bins * sizeof(int64_t), s));
    int64_t grid = ((n >> 2) + kThreads - 1) / kThreads;  // a workgroup's 32-bit counters see at most max(2^40 / grid, 4 * kThreads) voxels
    if (grid > persistent_workgroups()) grid = persistent_workgroups();
    if (grid < 1) grid = 1;
    hipLaunchKernelGGL(distance_histogram_kernel, dim3((unsigned)grid), dim3(kThreads), 0, s, from_surface, d2, n, bins,
                       (unsigned long long*)hist);
    VS_LAUNCH_CHECK();
    return VS_OK;
}
