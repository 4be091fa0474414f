// Local thickness of one value of a label volume (gfx950): from R, the exact squared distance of every voxel of the value to the
// nearest voxel of another value (vs_edt_squared with seeds = labels != value; R is 0 off the value), the map T2(u) = the largest
// R(v) over the voxels v whose open ball |u - v|^2 < R(v) contains u.  Integer arithmetic throughout and maxima only, so the
// result is the same bits on every run whatever order the atomics arrive in (utilities/thickness.py states the definitions).
//
// vs_thickness_centres: one sweep over R.  A voxel is dropped when one of its 26 neighbours has a ball that contains its own:
// R(n) >= need[faces | edges | corners][R(v)], three rows of a table the host builds (1 + the largest |p - delta|^2 over the
// lattice points p of the ball).  Such a neighbour has a strictly larger R, so chains of drops end at a kept voxel whose ball
// contains them all.  The kept voxels are appended to a list, one 64-bit add per workgroup and 1024 voxels; the list's order is
// whatever the workgroups' arrival gives, which a maximum does not see.  The same sweep adds up the rows the kept balls will paint.
//
// vs_thickness_paint: a ball is one x-span per row (dz, dy): m = R - dz^2 - dy^2 >= 1, half width h = the largest integer with
// h^2 < m (a float square root corrected by integer compares).  A span of length L goes into a sparse table of range maxima:
// with k = floor(log2 L), level k gets an atomic maximum at the span's first position and at its last position - 2^k + 1 (entry p of
// level k covers [p, p + 2^k)): two no-return 32-bit atomics per span instead of L, each behind a plain load that skips it when
// the entry is already as large - a stale load only issues an atomic that changes nothing, for entries never decrease.
// One lane per span, one centre per lane: a workgroup takes 64 consecutive centres of the list and its waves walk the rows (dz, dy) of
// the batch's widest ball, so the row offset, its dz^2 + dy^2 and the test against the widest ball are uniform over a wave, and a
// lane whose own ball does not reach the row idles for that step.  The caller orders the list by size class and, inside a class,
// by voxel index: a batch then holds balls of about one size - five-row balls share a wave 64 at a time - and mostly x-neighbours,
// whose spans on one row (z + dz, y + dy) start and end in the same cache lines.  gridDim.y workgroups share one batch (each takes
// every gridDim.y-th plane dz), sized by the launcher from the largest ball of the call so that no wave walks more than a few
// dozen rows.
//
// vs_thickness_resolve: level k - 1 takes, at x, the maximum of itself, level k at x and level k at x - 2^(k-1), from the top level
// down - a gather within a row, no atomics, one streaming launch per level.  The last launch also writes T2 = level 0 at the voxels
// of the value and leaves the other voxels of T2 alone.
#include "common.h"

namespace {

constexpr uint32_t kInf = 0xFFFFFFFFu;
constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kItems = 4;             // voxels per thread and step of the centres sweep
constexpr int kBatch = 64;            // centres of one paint workgroup: one per lane
constexpr int kWaveRows = 16;         // rows (dz, dy) a wave walks when the batch's widest ball is the call's largest
constexpr int kMaxSlices = 4096;      // most workgroups that share one batch

// the largest h with h * h <= v
__host__ __device__ inline uint32_t isqrt_u32(uint32_t v) {
    uint32_t h = (uint32_t)sqrtf((float)v);
    if (h > 65535u) h = 65535u;
    while ((uint64_t)h * h > v) --h;
    while ((uint64_t)(h + 1) * (h + 1) <= v) ++h;
    return h;
}

// n < 2^31 voxels and the extents vs_edt_squared takes: every squared distance below 2^32 - 1
bool thickness_extents_fit(int64_t Z, int64_t Y, int64_t X) {
    if (!extents_fit(Z, Y, X, 0) || Z > 65536 || Y > 65536 || X > 65536) return false;
    const uint64_t s = (uint64_t)((Z - 1) * (Z - 1)) + (uint64_t)((Y - 1) * (Y - 1)) + (uint64_t)((X - 1) * (X - 1));
    return s < 0xFFFFFFFFull;
}

// the squared steps of the grid along z, y, x: q = w^2, w the integer weights of the _scaled entry points; 1, 1, 1 otherwise
struct Steps { uint32_t qz, qy, qx; };
constexpr Steps kUnit = {1u, 1u, 1u};

// fewer than 2^31 voxels, weights 1..64, and the extents vs_edt_squared_scaled takes
bool scaled_extents_fit(int64_t Z, int64_t Y, int64_t X, int wz, int wy, int wx) {
    return thickness_extents_fit(Z, Y, X) && weighted_distances_fit(Z, Y, X, wz, wy, wx);
}

Steps steps_of(int wz, int wy, int wx) { return Steps{(uint32_t)(wz * wz), (uint32_t)(wy * wy), (uint32_t)(wx * wx)}; }

// levels of the sparse table: bit_length(min(2 h + 1, X)), h the half width of the widest span of a ball of squared radius max_r:
// the largest h with qx h^2 < max_r
int table_levels(int64_t X, uint32_t max_r, uint32_t qx = 1u) {
    int64_t longest = 2 * (int64_t)isqrt_u32((max_r - 1) / qx) + 1;
    if (longest > X) longest = X;
    int k = 0;
    while (longest) { ++k; longest >>= 1; }
    return k;
}

// rows (dz, dy) of the bounding rectangle of a ball that reaches hz planes and hy lines from (z, y), clipped to the volume
__device__ __forceinline__ void ball_rows(int z, int y, int hz, int hy, int Z, int Y, int& z0, int& y0, int& nz, int& ny) {
    z0 = z - hz > 0 ? z - hz : 0;
    y0 = y - hy > 0 ? y - hy : 0;
    const int z1 = (int64_t)z + hz < Z - 1 ? z + hz : Z - 1, y1 = (int64_t)y + hy < Y - 1 ? y + hy : Y - 1;
    nz = z1 - z0 + 1;
    ny = y1 - y0 + 1;
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// ---- centres ---------------------------------------------------------------------------------------------------------------------
// whether voxel i is a centre; the rows its ball will paint are added to spans.  kScaled: need has 7 rows, one per non-empty set
// of axes on which the neighbour's offset is non-zero (row 4 [z] + 2 [y] + [x] - 1), and the ball reaches isqrt((R - 1) / q) rows.
template <bool kScaled>
__device__ __forceinline__ bool is_centre(const uint32_t* __restrict__ r, int64_t i, int Z, int Y, int X, int64_t n, int64_t plane,
                                          const uint32_t* __restrict__ need, uint32_t need_len, Steps q, unsigned long long& spans) {
    const uint32_t rv = i < n ? r[i] : 0u;
    if (rv == 0u || rv == kInf) return false;
    const int64_t line = i / X;
    const int x = (int)(i - line * X), z = (int)(line / Y);
    const int y = (int)(line - (int64_t)z * Y);
    if (rv < need_len) {
        uint32_t thr[kScaled ? 7 : 3];
#pragma unroll
        for (int j = 0; j < (kScaled ? 7 : 3); ++j) thr[j] = need[j * (size_t)need_len + rv];
        bool keep = true;
#pragma unroll
        for (int dz = -1; dz <= 1; ++dz) {
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                    // unscaled: 1 = across a face, 2 = an edge, 3 = a corner; scaled: the set of axes the offset moves along
                    const int cls = kScaled ? 4 * (dz != 0) + 2 * (dy != 0) + (dx != 0) : (dz != 0) + (dy != 0) + (dx != 0);
                    if (cls == 0) continue;
                    const int zz = z + dz, yy = y + dy, xx = x + dx;
                    if (zz < 0 || zz >= Z || yy < 0 || yy >= Y || xx < 0 || xx >= X) continue;
                    if (keep && r[i + dz * plane + dy * (int64_t)X + dx] >= thr[cls - 1]) keep = false;
                }
            }
        }
        if (!keep) return false;
    }
    int z0, y0, nz, ny;
    if (kScaled) ball_rows(z, y, (int)isqrt_u32((rv - 1u) / q.qz), (int)isqrt_u32((rv - 1u) / q.qy), Z, Y, z0, y0, nz, ny);
    else { const int h = (int)isqrt_u32(rv - 1u); ball_rows(z, y, h, h, Z, Y, z0, y0, nz, ny); }
    spans += (unsigned long long)nz * (unsigned long long)ny;
    return true;
}

// A workgroup looks at kItems x kThreads consecutive voxels per step and takes its place in the list with ONE 64-bit add: returning
// atomics on one address queue up whoever issues them, and one per wave of 64 voxels was most of this sweep's time.
template <bool kScaled>
__global__ __launch_bounds__(kThreads) void thickness_centres_kernel(const uint32_t* __restrict__ r, int Z, int Y, int X, int64_t n,
                                                                   const uint32_t* __restrict__ need, uint32_t need_len,
                                                                   int32_t* __restrict__ centres, int64_t capacity,
                                                                   unsigned long long* __restrict__ totals, Steps q) {
    __shared__ unsigned long long wave_first[kWaves];          // in: the wave's count; out: the wave's first place
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t plane = (int64_t)Y * X, step = (int64_t)kItems * kThreads;
    unsigned long long spans = 0;
    for (int64_t base = (int64_t)blockIdx.x * step; base < n; base += (int64_t)gridDim.x * step) {              // uniform over the block
        unsigned long long mask[kItems];
        int mine = 0;
#pragma unroll
        for (int u = 0; u < kItems; ++u) {
            mask[u] = __ballot(is_centre<kScaled>(r, base + u * kThreads + threadIdx.x, Z, Y, X, n, plane, need, need_len, q, spans));
            mine += __popcll(mask[u]);
        }
        if (lane == 0) wave_first[wave] = (unsigned long long)mine;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned long long sum = 0;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) sum += wave_first[w];
            unsigned long long first = sum ? atomicAdd(&totals[0], sum) : 0ull;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) {
                const unsigned long long c = wave_first[w];
                wave_first[w] = first;
                first += c;
            }
        }
        __syncthreads();
        unsigned long long pos = wave_first[wave];
#pragma unroll
        for (int u = 0; u < kItems; ++u) {
            if ((mask[u] >> lane) & 1ull) {
                const unsigned long long at = pos + (unsigned long long)__popcll(mask[u] & ((1ull << lane) - 1ull));
                if (at < (unsigned long long)capacity) centres[at] = (int32_t)(base + u * kThreads + threadIdx.x);
            }
            pos += (unsigned long long)__popcll(mask[u]);
        }
        __syncthreads();                                       // wave_first is written again in the next step
    }
    spans = wave_sum_u64(spans);
    if (lane == 0 && spans) atomicAdd(&totals[1], spans);
}

// ---- painting --------------------------------------------------------------------------------------------------------------------
// kScaled: row (dz, dy) lies qz dz^2 + qy dy^2 off the centre and its half width is the largest h with qx h^2 < m
template <bool kScaled>
__global__ __launch_bounds__(kThreads) void thickness_paint_kernel(const uint32_t* __restrict__ r, int Z, int Y, int X, int64_t n,
                                                                 const int32_t* __restrict__ centres, int64_t count, uint32_t* levels,
                                                                 int K, Steps q) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // every wave of the workgroup holds the same 64 centres, one per lane
    const int64_t c = (int64_t)blockIdx.x * kBatch + lane;
    const int64_t i = c < count ? (int64_t)centres[c] : -1;
    uint32_t rv = i >= 0 && i < n ? r[i] : 0u;
    if (rv == kInf) rv = 0u;
    int x = 0, y = 0, z = 0, h = -1;
    if (rv) {
        const int64_t line = i / X;
        x = (int)(i - line * X);
        z = (int)(line / Y);
        y = (int)(line - (int64_t)z * Y);
        h = (int)isqrt_u32(rv - 1u);
    }
    int reach = h;                                    // the batch's widest ball: its rows are the rows every lane walks
    uint32_t largest = rv;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int t = __shfl_xor(reach, o, 64);
        const uint32_t u = __shfl_xor(largest, o, 64);
        reach = t > reach ? t : reach;
        largest = u > largest ? u : largest;
    }
    if (reach < 0) return;
    // the rows of the batch's widest ball; no row further than the volume is long
    const int rz = kScaled ? (int)isqrt_u32((largest - 1u) / q.qz) : reach, ry = kScaled ? (int)isqrt_u32((largest - 1u) / q.qy) : reach;
    const int hz = rz < Z - 1 ? rz : Z - 1, hy = ry < Y - 1 ? ry : Y - 1;
    for (int dz = -hz + (int)blockIdx.y; dz <= hz; dz += (int)gridDim.y) {                  // uniform over the workgroup
        for (int dy = -hy + wave; dy <= hy; dy += kWaves) {                                 // uniform over the wave
            const uint64_t off2 = kScaled ? (uint64_t)q.qz * (uint64_t)((int64_t)dz * dz) + (uint64_t)q.qy * (uint64_t)((int64_t)dy * dy)
                                          : (uint64_t)((int64_t)dz * dz + (int64_t)dy * dy);
            if (off2 >= largest) continue;            // outside the batch's widest ball
            const int zz = z + dz, yy = y + dy;
            if (off2 >= rv || zz < 0 || zz >= Z || yy < 0 || yy >= Y) continue;          // m = R - dz^2 - dy^2 < 1, or no such row
            // the largest h with h^2 < m; scaled: with qx h^2 < m, isqrt((m - 1) / qx)
            const int hs = (int)isqrt_u32(kScaled ? (rv - (uint32_t)off2 - 1u) / q.qx : rv - (uint32_t)off2 - 1u);
            const int first = x - hs > 0 ? x - hs : 0, last = x + hs < X - 1 ? x + hs : X - 1;
            const int k = 31 - __clz(last - first + 1);
            if (k >= K) continue;                     // cannot happen while max_r bounds every R: no store outside the table
            uint32_t* row = levels + (size_t)k * (size_t)n + ((size_t)zz * Y + yy) * (size_t)X;
            if (row[first] < rv) atomicMax(row + first, rv);
            const int second = last - (1 << k) + 1;
            if (second != first && row[second] < rv) atomicMax(row + second, rv);
        }
    }
}

// ---- resolve ---------------------------------------------------------------------------------------------------------------------
// lo = level k - 1, hi = level k (or null: there is one level), half = 2^(k-1); t2 (or null) is written where labels == value
__global__ __launch_bounds__(kThreads) void thickness_resolve_kernel(const uint32_t* __restrict__ hi, uint32_t* __restrict__ lo, int64_t n, int X,
                                                                   int half, const uint8_t* __restrict__ labels, int value,
                                                                   uint32_t* __restrict__ t2) {
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
        uint32_t v = lo[i];
        if (hi) {
            const uint32_t a = hi[i];
            v = a > v ? a : v;
            if ((int)(i % X) >= half) {
                const uint32_t b = hi[i - half];
                v = b > v ? b : v;
            }
            lo[i] = v;
        }
        if (t2 && labels[i] == (uint8_t)value) t2[i] = v;
    }
}

int sweep_grid(int64_t n) {
    int64_t grid = (n + kThreads - 1) / kThreads;
    if (grid > persistent_workgroups()) grid = persistent_workgroups();
    return (int)(grid < 1 ? 1 : grid);
}

// ---- the entry points, unscaled and scaled: one body each -------------------------------------------------------------------------
size_t workspace_bytes_of(int64_t Z, int64_t Y, int64_t X, int64_t max_r, Steps q) {
    if (!thickness_extents_fit(Z, Y, X) || max_r < 1 || max_r >= (int64_t)kInf) return 0;
    return (size_t)table_levels(X, (uint32_t)max_r, q.qx) * (size_t)(Z * Y * X) * sizeof(uint32_t);
}

template <bool kScaled>
int centres_impl(const uint32_t* r, int64_t Z, int64_t Y, int64_t X, const uint32_t* need, int64_t need_len, int32_t* centres, int64_t capacity,
                 int64_t* totals, Steps q, void* stream) {
    VS_REQUIRE(thickness_extents_fit(Z, Y, X),
               "thickness_centres: extents %lld x %lld x %lld - fewer than 2^31 voxels and (Z-1)^2 + (Y-1)^2 + (X-1)^2 below 2^32 - 1",
               (long long)Z, (long long)Y, (long long)X);
    VS_REQUIRE(r && totals && (centres || capacity == 0), "thickness_centres: null argument");
    VS_REQUIRE(need_len >= 0 && need_len < (int64_t)kInf && (need || need_len == 0), "thickness_centres: a table of %lld entries per row without a table, or too long",
               (long long)need_len);
    VS_REQUIRE(capacity >= 0, "thickness_centres: capacity %lld", (long long)capacity);
    VS_REQUIRE((uintptr_t)r % 4 == 0 && (uintptr_t)need % 4 == 0 && (uintptr_t)centres % 4 == 0 && (uintptr_t)totals % 8 == 0,
               "thickness_centres: r, need and centres must be 4-byte, totals 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    VS_CHECK_HIP(hipMemsetAsync(totals, 0, 2 * sizeof(int64_t), s));
    const int64_t n = Z * Y * X;
    hipLaunchKernelGGL(thickness_centres_kernel<kScaled>, dim3((unsigned)sweep_grid((n + kItems - 1) / kItems)), dim3(kThreads), 0, s, r, (int)Z, (int)Y, (int)X,
                       n, need, (uint32_t)need_len, centres, capacity, (unsigned long long*)totals, q);
    VS_LAUNCH_CHECK();
    return VS_OK;
}

template <bool kScaled>
int paint_impl(const uint32_t* r, int64_t Z, int64_t Y, int64_t X, const int32_t* centres, int64_t count, int64_t largest_r, int64_t max_r,
               void* workspace, size_t workspace_bytes, int zero_first, Steps q, void* stream) {
    VS_REQUIRE(thickness_extents_fit(Z, Y, X),
               "thickness_paint: extents %lld x %lld x %lld - fewer than 2^31 voxels and (Z-1)^2 + (Y-1)^2 + (X-1)^2 below 2^32 - 1",
               (long long)Z, (long long)Y, (long long)X);
    VS_REQUIRE(max_r >= 1 && max_r < (int64_t)kInf && largest_r >= 1 && largest_r <= max_r,
               "thickness_paint: squared radii %lld (this call's largest) and %lld (the volume's) - 1 <= largest <= the volume's < 2^32 - 1",
               (long long)largest_r, (long long)max_r);
    const int64_t n = Z * Y * X;
    VS_REQUIRE(count >= 0 && count <= n, "thickness_paint: %lld centres in a volume of %lld voxels", (long long)count, (long long)n);
    VS_REQUIRE(r && workspace && (centres || count == 0), "thickness_paint: null argument");
    const size_t need_bytes = workspace_bytes_of(Z, Y, X, max_r, q);
    VS_REQUIRE(workspace_bytes >= need_bytes, "thickness_paint: workspace of %zu bytes, %zu needed (vs_thickness_workspace_bytes)", workspace_bytes,
               need_bytes);
    VS_REQUIRE((uintptr_t)r % 4 == 0 && (uintptr_t)centres % 4 == 0 && (uintptr_t)workspace % 4 == 0,
               "thickness_paint: r, centres and workspace must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (zero_first) VS_CHECK_HIP(hipMemsetAsync(workspace, 0, need_bytes, s));
    if (count == 0) return VS_OK;
    // the rows of the call's largest ball decide how many workgroups share a batch: each takes every gridDim.y-th plane dz
    const int64_t rz = (int64_t)isqrt_u32(((uint32_t)largest_r - 1u) / q.qz), ry = (int64_t)isqrt_u32(((uint32_t)largest_r - 1u) / q.qy);
    const int64_t planes = 2 * (rz < Z - 1 ? rz : Z - 1) + 1, lines = 2 * (ry < Y - 1 ? ry : Y - 1) + 1;
    int64_t slices = (planes * lines + (int64_t)kWaves * kWaveRows - 1) / ((int64_t)kWaves * kWaveRows);
    if (slices < 1) slices = 1;
    if (slices > planes) slices = planes;
    if (slices > kMaxSlices) slices = kMaxSlices;
    const int64_t batches = (count + kBatch - 1) / kBatch;
    hipLaunchKernelGGL(thickness_paint_kernel<kScaled>, dim3((unsigned)batches, (unsigned)slices), dim3(kThreads), 0, s, r, (int)Z, (int)Y, (int)X, n,
                       centres, count, (uint32_t*)workspace, table_levels(X, (uint32_t)max_r, q.qx), q);
    VS_LAUNCH_CHECK();
    return VS_OK;
}

int resolve_impl(const uint8_t* labels, int64_t Z, int64_t Y, int64_t X, int value, int64_t max_r, void* workspace, size_t workspace_bytes,
                 uint32_t* t2, Steps q, void* stream) {
    VS_REQUIRE(thickness_extents_fit(Z, Y, X),
               "thickness_resolve: extents %lld x %lld x %lld - fewer than 2^31 voxels and (Z-1)^2 + (Y-1)^2 + (X-1)^2 below 2^32 - 1",
               (long long)Z, (long long)Y, (long long)X);
    VS_REQUIRE(value >= 0 && value <= 255, "thickness_resolve: value %d is not a uint8 value", value);
    VS_REQUIRE(max_r >= 1 && max_r < (int64_t)kInf, "thickness_resolve: squared radius %lld - 1 <= max_r < 2^32 - 1", (long long)max_r);
    VS_REQUIRE(labels && workspace && t2, "thickness_resolve: null argument");
    const size_t need_bytes = workspace_bytes_of(Z, Y, X, max_r, q);
    VS_REQUIRE(workspace_bytes >= need_bytes, "thickness_resolve: workspace of %zu bytes, %zu needed (vs_thickness_workspace_bytes)", workspace_bytes,
               need_bytes);
    VS_REQUIRE((uintptr_t)workspace % 4 == 0 && (uintptr_t)t2 % 4 == 0, "thickness_resolve: workspace and t2 must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = Z * Y * X;
    const int K = table_levels(X, (uint32_t)max_r, q.qx);
    uint32_t* levels = (uint32_t*)workspace;
    const dim3 grid((unsigned)sweep_grid(n));
    if (K == 1) {
        hipLaunchKernelGGL(thickness_resolve_kernel, grid, dim3(kThreads), 0, s, (const uint32_t*)nullptr, levels, n, (int)X, 0, labels, value, t2);
        VS_LAUNCH_CHECK();
    }
    for (int k = K - 1; k >= 1; --k) {
        hipLaunchKernelGGL(thickness_resolve_kernel, grid, dim3(kThreads), 0, s, (const uint32_t*)(levels + (size_t)k * n), levels + (size_t)(k - 1) * n, n,
                           (int)X, 1 << (k - 1), labels, value, k == 1 ? t2 : (uint32_t*)nullptr);
        VS_LAUNCH_CHECK();
    }
    return VS_OK;
}

}  // namespace

#define VS_REQUIRE_WEIGHTS(what)                                                                                                              \
    VS_REQUIRE(scaled_extents_fit(Z, Y, X, wz, wy, wx),                                                                                        \
               what ": extents %lld x %lld x %lld under weights %d, %d, %d - fewer than 2^31 voxels, every weight 1..64 and wz^2 (Z-1)^2 + "  \
                    "wy^2 (Y-1)^2 + wx^2 (X-1)^2 below 2^32 - 1",                                                                             \
               (long long)Z, (long long)Y, (long long)X, wz, wy, wx)

extern "C" size_t vs_thickness_workspace_bytes(int64_t Z, int64_t Y, int64_t X, int64_t max_r) { return workspace_bytes_of(Z, Y, X, max_r, kUnit); }

extern "C" size_t vs_thickness_workspace_bytes_scaled(int64_t Z, int64_t Y, int64_t X, int wz, int wy, int wx, int64_t max_r) {
    return scaled_extents_fit(Z, Y, X, wz, wy, wx) ? workspace_bytes_of(Z, Y, X, max_r, steps_of(wz, wy, wx)) : 0;
}

extern "C" int vs_thickness_centres(const uint32_t* r, int64_t Z, int64_t Y, int64_t X, const uint32_t* need, int64_t need_len,
                                    int32_t* centres, int64_t capacity, int64_t* totals, void* stream) {
    return centres_impl<false>(r, Z, Y, X, need, need_len, centres, capacity, totals, kUnit, stream);
}

extern "C" int vs_thickness_centres_scaled(const uint32_t* r, int64_t Z, int64_t Y, int64_t X, int wz, int wy, int wx, const uint32_t* need,
                                           int64_t need_len, int32_t* centres, int64_t capacity, int64_t* totals, void* stream) {
    VS_REQUIRE_WEIGHTS("thickness_centres_scaled");
    return centres_impl<true>(r, Z, Y, X, need, need_len, centres, capacity, totals, steps_of(wz, wy, wx), stream);
}

extern "C" int vs_thickness_paint(const uint32_t* r, int64_t Z, int64_t Y, int64_t X, const int32_t* centres, int64_t count, int64_t largest_r,
                                  int64_t max_r, void* workspace, size_t workspace_bytes, int zero_first, void* stream) {
    return paint_impl<false>(r, Z, Y, X, centres, count, largest_r, max_r, workspace, workspace_bytes, zero_first, kUnit, stream);
}

extern "C" int vs_thickness_paint_scaled(const uint32_t* r, int64_t Z, int64_t Y, int64_t X, int wz, int wy, int wx, const int32_t* centres,
                                         int64_t count, int64_t largest_r, int64_t max_r, void* workspace, size_t workspace_bytes, int zero_first,
                                         void* stream) {
    VS_REQUIRE_WEIGHTS("thickness_paint_scaled");
    return paint_impl<true>(r, Z, Y, X, centres, count, largest_r, max_r, workspace, workspace_bytes, zero_first, steps_of(wz, wy, wx), stream);
}

extern "C" int vs_thickness_resolve(const uint8_t* labels, int64_t Z, int64_t Y, int64_t X, int value, int64_t max_r, void* workspace,
                                    size_t workspace_bytes, uint32_t* t2, void* stream) {
    return resolve_impl(labels, Z, Y, X, value, max_r, workspace, workspace_bytes, t2, kUnit, stream);
}

extern "C" int vs_thickness_resolve_scaled(const uint8_t* labels, int64_t Z, int64_t Y, int64_t X, int wz, int wy, int wx, int value, int64_t max_r,
                                           void* workspace, size_t workspace_bytes, uint32_t* t2, void* stream) {
    VS_REQUIRE_WEIGHTS("thickness_resolve_scaled");
    return resolve_impl(labels, Z, Y, X, value, max_r, workspace, workspace_bytes, t2, steps_of(wz, wy, wx), stream);
}
