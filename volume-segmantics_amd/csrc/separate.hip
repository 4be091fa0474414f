// Distance-map watershed of one label value (gfx950): the stages that take touching objects apart (include/volseg_hip.h has the
// contract; utilities/separation.py is the Python layer, the shared host merge and the host route that gives the same integers).
// r is the squared distance of every voxel of the value to the nearest voxel of another value (vs_edt_squared), 0 off the value.
// The key of a voxel is (r << 32) | (0xFFFFFFFF - index): all keys differ, the higher r wins, then the lower index.  Exact
// integers throughout; maxima, minima and integer adds commute, so atomics are allowed and every result is the same bits on every
// run.  Every stage is a bounded sweep: no kernel waits on another workgroup and there is no host loop.
//
// All stencil stages work on the tile of components.hip, kTZ x kTY x kTX = 8 x 8 x 64 voxels, staged in LDS with a halo of one
// voxel (10 x 10 x 66 entries; outside the volume reads r = 0 / basin = -1, so an axis of length 1 has no neighbours); a wave owns
// a row of 64 voxels along x.
//
// vs_separate_parents: parent[v] = the voxel with the largest key among v and its 6 / 18 / 26 neighbours, -1 where r[v] == 0.  A
//  neighbour off the value has r = 0 and never wins, so r alone is read: up to 26 LDS reads per voxel, one global read.
// vs_separate_basins, in place, two launches:
//  1 tile_kernel: the pointers of a tile go to LDS - a pointer that stays in the tile as a local index, one that leaves as the mark
//    -2 - target - and are jumped, p[i] = p[p[i]], until nothing changes: a round at least halves what is left of every chain inside
//    the tile, so kJumpRounds = 13 rounds serve 4096 voxels.  Written back: the peak where the chain ends in the tile, else the
//    first voxel outside the tile.  A plateau's long diagonal walk costs log2 rounds here, not its length.
//  2 follow_kernel: every voxel follows what is left - one hop per visit to a tile - to the peak and writes it back.  Keys strictly
//    increase along a chain, so every walk ends on any output of vs_separate_parents (and after n hops on anything else).  A
//    walker may read a pointer that another workgroup has already shortened: what it reads is still a voxel further along the
//    same chain - the peak at best - so a stale read costs a hop, never a wrong peak; the 32-bit loads and stores are atomic.
//    Workgroups start in index order and a plateau's chains run towards index 0, so most walks end after one or two hops on a
//    pointer that was already written back.
// vs_separate_pair_count: adjacent voxel pairs in different basins, each counted at its later voxel (3 / 9 / 13 forward offsets);
//  one 64-bit add per workgroup.
// vs_separate_pairs: the table of (lower peak << 32 | higher peak) -> (saddle = max of min(r, r), faces across z, y, x), open
//  addressing with linear probing as in overlap.hip: read the slot, compare-and-swap the key into a free one, then a 32-bit
//  atomicMax and up to one 32-bit add; `slots` probes at most, then used[1] = 1 and the lane gives up.  The table is tiny
//  against what is inserted, so a wave aggregates: per forward offset the lanes that hold one key are found by ballot (kRounds keys
//  per offset, the rest - debris - insert on their own, on addresses the hash spreads), their saddle is reduced by shuffles and
//  the result goes to the wave's cache - one entry per LANE, in registers, two ways - which a key leaves when another takes its
//  lane and at the end of the wave's 16 rows.  The border between two big basins costs one insertion per wave and tile.
// vs_separate_relabel: two sweeps.  The lowest voxel of every merged set (workspace[representative peak], atomicMin by the first
//  lane of the wave that holds the representative - lanes ascend with the index - and only where the slot still reads higher),
//  then objects[v] = that voxel wherever basin[v] >= 0.
#include <limits.h>

#include "common.h"
#include "prof.h"

namespace {

constexpr int kTZ = 8, kTY = 8, kTX = 64;      // tile extents, as in components.hip
constexpr int kRows = kTZ * kTY, kTile = kRows * kTX;
constexpr int kHY = kTY + 2, kHX = kTX + 2, kHalo = (kTZ + 2) * kHY * kHX;      // 6600 entries: 26.4 KB of 32-bit values
constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kJumpRounds = 13;                // 2^12 = kTile: a chain inside a tile is resolved after 12 halvings
constexpr int kRounds = 4;                     // keys per forward offset (representatives per 64 voxels) a wave groups by ballot
constexpr unsigned long long kFree = ~0ull;    // no key: peaks are below 2^31

struct Grid {                                  // the volume and its tiling
    int Z, Y, X, ny, nx;
};
Grid make_grid(int64_t Z, int64_t Y, int64_t X) { return Grid{(int)Z, (int)Y, (int)X, (int)((Y + kTY - 1) / kTY), (int)((X + kTX - 1) / kTX)}; }
int64_t tiles_of(int64_t Z, int64_t Y, int64_t X) { return ((Z + kTZ - 1) / kTZ) * ((Y + kTY - 1) / kTY) * ((X + kTX - 1) / kTX); }

struct Origin {
    int z0, y0, x0;
};
__device__ __forceinline__ Origin origin_of(const Grid& g, int t) {
    const int bx = t % g.nx;
    t /= g.nx;
    return Origin{(t / g.ny) * kTZ, (t % g.ny) * kTY, bx * kTX};
}

// how many of the three offsets may be non-zero
int reach_of(int connectivity) { return connectivity == 6 ? 1 : connectivity == 18 ? 2 : 3; }

// the tile and its halo: entry ((tz + 1) * kHY + ty + 1) * kHX + tx + 1 is voxel (z0 + tz, y0 + ty, x0 + tx), `outside` beyond the volume
template <typename T>
__device__ __forceinline__ void load_halo(const T* __restrict__ src, const Grid& g, const Origin& o, T outside, T* tile) {
    for (int i = threadIdx.x; i < kHalo; i += kThreads) {
        const int z = o.z0 + i / (kHX * kHY) - 1, y = o.y0 + (i / kHX) % kHY - 1, x = o.x0 + i % kHX - 1;
        const bool in = z >= 0 && z < g.Z && y >= 0 && y < g.Y && x >= 0 && x < g.X;
        tile[i] = in ? src[((int64_t)z * g.Y + y) * g.X + x] : outside;
    }
}
__device__ __forceinline__ int halo_at(int tz, int ty, int tx) { return ((tz + 1) * kHY + ty + 1) * kHX + tx + 1; }

// ---- parents -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void parents_kernel(const uint32_t* __restrict__ r, Grid g, int reach, int* __restrict__ parent) {
    __shared__ uint32_t tile[kHalo];
    const Origin o = origin_of(g, blockIdx.x);
    load_halo(r, g, o, 0u, tile);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int row = wave; row < kRows; row += kWaves) {                    // uniform over the wave
        const int tz = row / kTY, ty = row % kTY;
        const int z = o.z0 + tz, y = o.y0 + ty, x = o.x0 + lane;
        if (z >= g.Z || y >= g.Y || x >= g.X) continue;
        const int64_t v = ((int64_t)z * g.Y + y) * g.X + x;
        uint32_t best_r = tile[halo_at(tz, ty, lane)];
        int best = -1;
        if (best_r) {
            best = (int)v;
#pragma unroll
            for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
                for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                    for (int dx = -1; dx <= 1; ++dx) {
                        const int nonzero = (dz != 0) + (dy != 0) + (dx != 0);
                        if (nonzero == 0 || nonzero > reach) continue;     // uniform
                        const uint32_t nr = tile[halo_at(tz + dz, ty + dy, lane + dx)];
                        const int ni = (int)(v + ((int64_t)dz * g.Y + dy) * g.X + dx);      // read only where nr > 0: then it is in the volume
                        if (nr > best_r || (nr == best_r && ni < best)) { best_r = nr; best = ni; }
                    }
        }
        parent[v] = best;
    }
}

// ---- basins --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void basin_tile_kernel(int* __restrict__ parent, Grid g) {
    __shared__ int p[kTile];                   // >= 0: a voxel of this tile; -1: no pointer; <= -2: the voxel -2 - p outside the tile
    const Origin o = origin_of(g, blockIdx.x);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int row = wave; row < kRows; row += kWaves) {
        const int z = o.z0 + row / kTY, y = o.y0 + row % kTY, x = o.x0 + lane;
        int local = -1;
        if (z < g.Z && y < g.Y && x < g.X) {
            const int q = parent[((int64_t)z * g.Y + y) * g.X + x];
            if (q >= 0) {
                const uint32_t line = (uint32_t)q / (uint32_t)g.X;
                const int lx = (int)((uint32_t)q - line * (uint32_t)g.X) - o.x0, ly = (int)(line % (uint32_t)g.Y) - o.y0, lz = (int)(line / (uint32_t)g.Y) - o.z0;
                const bool inside = lx >= 0 && lx < kTX && ly >= 0 && ly < kTY && lz >= 0 && lz < kTZ;
                local = inside ? (lz * kTY + ly) * kTX + lx : -2 - q;      // q <= 2^31 - 2: the mark fits
            }
        }
        p[row * kTX + lane] = local;
    }
    __syncthreads();
    for (int round = 0; round < kJumpRounds; ++round) {
        int changed = 0;
        for (int i = threadIdx.x; i < kTile; i += kThreads) {
            const int j = __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (j < 0 || j == i) continue;
            const int pj = __hip_atomic_load(p + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);      // maybe already jumped: further along the same chain
            if (pj != j && pj != -1) {
                __hip_atomic_store(p + i, pj, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                changed = 1;
            }
        }
        if (!__syncthreads_or(changed)) break;
    }
    for (int row = wave; row < kRows; row += kWaves) {
        const int z = o.z0 + row / kTY, y = o.y0 + row % kTY, x = o.x0 + lane;
        if (z >= g.Z || y >= g.Y || x >= g.X) continue;
        const int j = p[row * kTX + lane];
        if (j == -1) continue;
        const int jr = j / kTX;
        parent[((int64_t)z * g.Y + y) * g.X + x] =
            j <= -2 ? -2 - j : (int)(((int64_t)(o.z0 + jr / kTY) * g.Y + (o.y0 + jr % kTY)) * g.X + o.x0 + j % kTX);
    }
}

__global__ __launch_bounds__(kThreads) void basin_follow_kernel(int* parent, int64_t n) {
    const int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (v >= n) return;
    int p = parent[v];
    if (p < 0 || p == (int)v || p >= n) return;
    for (int64_t hop = 0; hop < n; ++hop) {                              // ends long before: keys increase along the chain
        const int q = __hip_atomic_load(parent + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (q == p || q < 0 || q >= n) break;
        p = q;
    }
    __hip_atomic_store(parent + v, p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);       // a reader finds the old pointer or the peak: both on its chain
}

// ---- pairs ---------------------------------------------------------------------------------------------------------------------
// forward offset o = 0 .. 12: the neighbours that come before a voxel in index order
__device__ __forceinline__ void forward_offset(int o, int& dz, int& dy, int& dx) {
    if (o < 9) { dz = -1; dy = o / 3 - 1; dx = o % 3 - 1; }
    else if (o < 12) { dz = 0; dy = -1; dx = o - 10; }
    else { dz = 0; dy = 0; dx = -1; }
}

__global__ __launch_bounds__(kThreads) void pair_count_kernel(const int* __restrict__ basin, Grid g, int reach, unsigned long long* __restrict__ count) {
    __shared__ int tile[kHalo];
    __shared__ unsigned long long total;
    const Origin o = origin_of(g, blockIdx.x);
    if (threadIdx.x == 0) total = 0;
    load_halo(basin, g, o, -1, tile);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int mine = 0;
    for (int row = wave; row < kRows; row += kWaves) {
        const int tz = row / kTY, ty = row % kTY;
        if (o.z0 + tz >= g.Z || o.y0 + ty >= g.Y || o.x0 + lane >= g.X) continue;
        const int b = tile[halo_at(tz, ty, lane)];
        if (b < 0) continue;
#pragma unroll
        for (int k = 0; k < 13; ++k) {
            int dz, dy, dx;
            forward_offset(k, dz, dy, dx);
            if ((dz != 0) + (dy != 0) + (dx != 0) > reach) continue;
            const int nb = tile[halo_at(tz + dz, ty + dy, lane + dx)];
            mine += nb >= 0 && nb != b;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off, 64);
    if (lane == 0 && mine) atomicAdd(&total, (unsigned long long)mine);
    __syncthreads();
    if (threadIdx.x == 0 && total) atomicAdd(count, total);
}

__device__ __forceinline__ unsigned long long mix(unsigned long long h) {
    h ^= h >> 33; h *= 0xff51afd7ed558ccdull;
    h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53ull;
    return h ^ (h >> 33);
}

struct Table {
    unsigned long long* keys;
    uint32_t* saddle;
    int* faces;                                // three per slot
    unsigned long long mask;
    unsigned long long* used;
};

// (saddle, faces) into the row of `key`; returns 1 when this lane claimed a free slot.  At most mask + 1 probes, never a spin.
__device__ __forceinline__ int insert(const Table& t, unsigned long long key, uint32_t saddle, int fz, int fy, int fx) {
    unsigned long long slot = mix(key) & t.mask;
    for (unsigned long long probe = 0; probe <= t.mask; ++probe, slot = (slot + 1) & t.mask) {
        unsigned long long seen = __hip_atomic_load(t.keys + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        int claimed = 0;
        if (seen == kFree) {
            seen = atomicCAS(t.keys + slot, kFree, key);
            claimed = seen == kFree;
            if (claimed) seen = key;
        }
        if (seen == key) {
            atomicMax(t.saddle + slot, saddle);
            if (fz) atomicAdd(t.faces + 3 * slot, fz);
            if (fy) atomicAdd(t.faces + 3 * slot + 1, fy);
            if (fx) atomicAdd(t.faces + 3 * slot + 2, fx);
            return claimed;
        }
    }
    __hip_atomic_store(t.used + 1, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // the table is full: give up
    return 0;
}

__global__ __launch_bounds__(kThreads) void pairs_kernel(const uint32_t* __restrict__ r, const int* __restrict__ basin, Grid g, int reach, Table t) {
    __shared__ int tile_b[kHalo];
    __shared__ uint32_t tile_r[kHalo];
    const Origin o = origin_of(g, blockIdx.x);
    load_halo(basin, g, o, -1, tile_b);
    load_halo(r, g, o, 0u, tile_r);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long cached_key = kFree;                                // this lane's entry of the wave's cache
    uint32_t cached_saddle = 0;
    int cached_fz = 0, cached_fy = 0, cached_fx = 0, claims = 0;
    for (int row = wave; row < kRows; row += kWaves) {                    // uniform over the wave
        const int tz = row / kTY, ty = row % kTY;
        const bool valid = o.z0 + tz < g.Z && o.y0 + ty < g.Y && o.x0 + lane < g.X;
        const int b = valid ? tile_b[halo_at(tz, ty, lane)] : -1;
        if (!__ballot(b >= 0)) continue;                                  // uniform: 64 voxels off the value
        const uint32_t own = tile_r[halo_at(tz, ty, lane)];
#pragma unroll
        for (int k = 0; k < 13; ++k) {
            int dz, dy, dx;
            forward_offset(k, dz, dy, dx);
            const int nonzero = (dz != 0) + (dy != 0) + (dx != 0);
            if (nonzero > reach) continue;                                // uniform
            const int fz = nonzero == 1 && dz != 0, fy = nonzero == 1 && dy != 0, fx = nonzero == 1 && dx != 0;
            const int at = halo_at(tz + dz, ty + dy, lane + dx);
            const int nb = tile_b[at];
            const bool active = b >= 0 && nb >= 0 && nb != b;
            uint64_t rest = __ballot(active);
            if (!rest) continue;                                          // uniform
            const uint32_t lo = (uint32_t)(b < nb ? b : nb), hi = (uint32_t)(b < nb ? nb : b);
            const uint32_t nr = tile_r[at], saddle = own < nr ? own : nr;
            const unsigned long long key = ((unsigned long long)lo << 32) | hi;
            for (int round = 0; round < kRounds && rest; ++round) {      // uniform
                const int leader = __ffsll((unsigned long long)rest) - 1;
                const uint32_t want_lo = (uint32_t)__shfl((int)lo, leader, 64), want_hi = (uint32_t)__shfl((int)hi, leader, 64);
                const unsigned long long want = ((unsigned long long)want_lo << 32) | want_hi;
                const uint64_t same = __ballot(active && key == want);
                uint32_t top = ((same >> lane) & 1) ? saddle : 0u;
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) {
                    const uint32_t other = (uint32_t)__shfl_xor((int)top, off, 64);
                    top = other > top ? other : top;
                }
                // two ways: the key's home lane and its neighbour - the lane that holds the key, else a free one, else home
                const int home = (int)(((want_lo * 0x9E3779B1u) ^ (want_hi * 0x85EBCA6Bu)) >> 26);
                const bool way = (lane | 1) == (home | 1);
                const uint64_t holds = __ballot(way && cached_key == want), free_way = __ballot(way && cached_key == kFree);
                const int target = holds ? __ffsll((unsigned long long)holds) - 1 : free_way ? __ffsll((unsigned long long)free_way) - 1 : home;
                if (lane == target) {
                    if (cached_key != want) {
                        if (cached_key != kFree) claims += insert(t, cached_key, cached_saddle, cached_fz, cached_fy, cached_fx);
                        cached_key = want;
                        cached_saddle = 0;
                        cached_fz = cached_fy = cached_fx = 0;
                    }
                    const int members = __popcll(same);
                    cached_saddle = top > cached_saddle ? top : cached_saddle;
                    cached_fz += fz * members; cached_fy += fy * members; cached_fx += fx * members;
                }
                rest &= ~same;
            }
            if ((rest >> lane) & 1) claims += insert(t, key, saddle, fz, fy, fx);      // more than kRounds keys at one offset of 64 voxels: debris
        }
    }
    if (cached_key != kFree) claims += insert(t, cached_key, cached_saddle, cached_fz, cached_fy, cached_fx);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) claims += __shfl_xor(claims, off, 64);
    if (lane == 0 && claims) atomicAdd(t.used, (unsigned long long)claims);
}

// ---- relabel -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int representative(const int* __restrict__ basin, const int* __restrict__ set_of_peak, int64_t v, int64_t n) {
    const int b = v < n ? basin[v] : -1;
    const int rep = b >= 0 && b < n ? set_of_peak[b] : -1;
    return rep < n ? rep : -1;
}

__device__ __forceinline__ void lower(uint32_t* slot, uint32_t v) {
    if (__hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > v) atomicMin(slot, v);      // mostly read: the sweep ascends
}

__global__ __launch_bounds__(kThreads) void lowest_kernel(const int* __restrict__ basin, const int* __restrict__ set_of_peak, int64_t n, uint32_t* lowest) {
    const int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x;      // a wave holds 64 consecutive voxels: a group's first lane is its lowest
    const int lane = threadIdx.x & 63;
    const int rep = representative(basin, set_of_peak, v, n);
    uint64_t rest = __ballot(rep >= 0);
    for (int round = 0; round < kRounds && rest; ++round) {              // uniform
        const int leader = __ffsll((unsigned long long)rest) - 1;
        const int want = __shfl(rep, leader, 64);
        if (lane == leader) lower(lowest + want, (uint32_t)v);
        rest &= ~__ballot(rep == want);
    }
    if ((rest >> lane) & 1) lower(lowest + rep, (uint32_t)v);
}

__global__ __launch_bounds__(kThreads) void relabel_kernel(const int* __restrict__ basin, const int* __restrict__ set_of_peak, int64_t n,
                                                         const uint32_t* __restrict__ lowest, int* __restrict__ objects) {
    const int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int rep = representative(basin, set_of_peak, v, n);
    if (rep >= 0) objects[v] = (int)lowest[rep];
}

}  // namespace

#define VS_SEPARATE_EXTENTS(what)                                                                                                           \
    VS_REQUIRE(extents_fit(Z, Y, X, 0), what ": extents %lld x %lld x %lld - every extent must be at least 1 and the volume below 2^31 voxels " \
               "(basins and objects are int32 voxel indices)", (long long)Z, (long long)Y, (long long)X)
#define VS_SEPARATE_CONNECTIVITY(what) \
    VS_REQUIRE(connectivity == 6 || connectivity == 18 || connectivity == 26, what ": connectivity %d - it is 6, 18 or 26", connectivity)

extern "C" int vs_separate_parents(const uint32_t* r, int64_t Z, int64_t Y, int64_t X, int connectivity, int32_t* parent, void* stream) {
    VS_SEPARATE_EXTENTS("separate_parents");
    VS_SEPARATE_CONNECTIVITY("separate_parents");
    VS_REQUIRE(r && parent, "separate_parents: null argument");
    VS_REQUIRE(((uintptr_t)r | (uintptr_t)parent) % 4 == 0, "separate_parents: r and parent must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(PK_POOL_MISC, 0.0, 8.0 * (double)(Z * Y * X), s);
    hipLaunchKernelGGL(parents_kernel, dim3((unsigned)tiles_of(Z, Y, X)), dim3(kThreads), 0, s, r, make_grid(Z, Y, X),
                       reach_of(connectivity), parent);
    VS_LAUNCH_CHECK();
    return VS_OK;
}

extern "C" int vs_separate_basins(int32_t* parent, int64_t Z, int64_t Y, int64_t X, void* stream) {
    VS_SEPARATE_EXTENTS("separate_basins");
    VS_REQUIRE(parent && (uintptr_t)parent % 4 == 0, "separate_basins: parent must be 4-byte aligned device memory");
    const int64_t n = Z * Y * X;
    hipStream_t s = (hipStream_t)stream;
    {
        ProfScope prof(PK_POOL_MISC, 0.0, 8.0 * (double)n, s);
        hipLaunchKernelGGL(basin_tile_kernel, dim3((unsigned)tiles_of(Z, Y, X)), dim3(kThreads), 0, s, parent, make_grid(Z, Y, X));
        VS_LAUNCH_CHECK();
    }
    {
        ProfScope prof(PK_POOL_MISC, 0.0, 8.0 * (double)n, s);
        hipLaunchKernelGGL(basin_follow_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, parent, n);
        VS_LAUNCH_CHECK();
    }
    return VS_OK;
}

extern "C" int vs_separate_pair_count(const int32_t* basin, int64_t Z, int64_t Y, int64_t X, int connectivity, int64_t* count, void* stream) {
    VS_SEPARATE_EXTENTS("separate_pair_count");
    VS_SEPARATE_CONNECTIVITY("separate_pair_count");
    VS_REQUIRE(basin && count, "separate_pair_count: null argument");
    VS_REQUIRE((uintptr_t)basin % 4 == 0 && (uintptr_t)count % 8 == 0, "separate_pair_count: basin must be 4-byte, count 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    VS_CHECK_HIP(hipMemsetAsync(count, 0, sizeof(int64_t), s));
    ProfScope prof(PK_POOL_MISC, 0.0, 4.0 * (double)(Z * Y * X), s);
    hipLaunchKernelGGL(pair_count_kernel, dim3((unsigned)tiles_of(Z, Y, X)), dim3(kThreads), 0, s, basin, make_grid(Z, Y, X),
                       reach_of(connectivity), (unsigned long long*)count);
    VS_LAUNCH_CHECK();
    return VS_OK;
}

extern "C" int vs_separate_pairs(const uint32_t* r, const int32_t* basin, int64_t Z, int64_t Y, int64_t X, int connectivity, uint64_t* keys,
                                 uint32_t* saddle, int32_t* faces, int64_t slots, int64_t* used, void* stream) {
    VS_SEPARATE_EXTENTS("separate_pairs");
    VS_SEPARATE_CONNECTIVITY("separate_pairs");
    VS_REQUIRE(slots >= 1 && slots < (1LL << 40) && (slots & (slots - 1)) == 0, "separate_pairs: %lld slots - the table size is a power of two", (long long)slots);
    VS_REQUIRE(r && basin && keys && saddle && faces && used, "separate_pairs: null argument");
    VS_REQUIRE(((uintptr_t)r | (uintptr_t)basin | (uintptr_t)saddle | (uintptr_t)faces) % 4 == 0 && ((uintptr_t)keys | (uintptr_t)used) % 8 == 0,
               "separate_pairs: r, basin, saddle and faces must be 4-byte, keys and used 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    VS_CHECK_HIP(hipMemsetAsync(keys, 0xFF, (size_t)slots * sizeof(uint64_t), s));
    VS_CHECK_HIP(hipMemsetAsync(saddle, 0, (size_t)slots * sizeof(uint32_t), s));
    VS_CHECK_HIP(hipMemsetAsync(faces, 0, (size_t)slots * 3 * sizeof(int32_t), s));
    VS_CHECK_HIP(hipMemsetAsync(used, 0, 2 * sizeof(int64_t), s));
    {
        ProfScope prof(PK_POOL_MISC, 0.0, 8.0 * (double)(Z * Y * X), s);
        hipLaunchKernelGGL(pairs_kernel, dim3((unsigned)tiles_of(Z, Y, X)), dim3(kThreads), 0, s, r, basin, make_grid(Z, Y, X),
                           reach_of(connectivity),
                           Table{(unsigned long long*)keys, saddle, faces, (unsigned long long)(slots - 1), (unsigned long long*)used});
        VS_LAUNCH_CHECK();
    }
    int64_t host_used[2] = {0, 0};
    VS_CHECK_HIP(hipMemcpyAsync(host_used, used, sizeof(host_used), hipMemcpyDeviceToHost, s));
    VS_CHECK_HIP(hipStreamSynchronize(s));
    VS_REQUIRE(host_used[1] == 0, "separate_pairs: the table of %lld slots is full - an insertion found no slot for its pair of basins; size it from "
               "vs_separate_pair_count (a power of two at or above twice the smaller of the count and B (B - 1) / 2 for B basins)", (long long)slots);
    return VS_OK;
}

extern "C" size_t vs_separate_workspace_bytes(int64_t Z, int64_t Y, int64_t X) {
    return extents_fit(Z, Y, X, 0) ? (size_t)(Z * Y * X) * sizeof(int32_t) : 0;
}

extern "C" int vs_separate_relabel(const int32_t* basin, const int32_t* set_of_peak, int64_t Z, int64_t Y, int64_t X, int32_t* objects,
                                   void* workspace, size_t workspace_bytes, void* stream) {
    VS_SEPARATE_EXTENTS("separate_relabel");
    VS_REQUIRE(basin && set_of_peak && objects, "separate_relabel: null argument");
    const size_t need = vs_separate_workspace_bytes(Z, Y, X);
    VS_REQUIRE(workspace && workspace_bytes >= need, "separate_relabel: workspace of %zu bytes, %zu needed (vs_separate_workspace_bytes)",
               workspace ? workspace_bytes : (size_t)0, need);
    VS_REQUIRE(((uintptr_t)basin | (uintptr_t)set_of_peak | (uintptr_t)objects | (uintptr_t)workspace) % 4 == 0,
               "separate_relabel: basin, set_of_peak, objects and workspace must be 4-byte aligned");
    const int64_t n = Z * Y * X;
    hipStream_t s = (hipStream_t)stream;
    VS_CHECK_HIP(hipMemsetAsync(workspace, 0xFF, need, s));               // 0xFFFFFFFF: above every voxel index
    const unsigned grid = (unsigned)((n + kThreads - 1) / kThreads);
    {
        ProfScope prof(PK_POOL_MISC, 0.0, 8.0 * (double)n, s);
        hipLaunchKernelGGL(lowest_kernel, dim3(grid), dim3(kThreads), 0, s, basin, set_of_peak, n, (uint32_t*)workspace);
        VS_LAUNCH_CHECK();
    }
    {
        ProfScope prof(PK_POOL_MISC, 0.0, 12.0 * (double)n, s);
        hipLaunchKernelGGL(relabel_kernel, dim3(grid), dim3(kThreads), 0, s, basin, set_of_peak, n, (const uint32_t*)workspace, objects);
        VS_LAUNCH_CHECK();
    }
    return VS_OK;
}
