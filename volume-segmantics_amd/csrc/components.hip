// Connected components of a uint8 label volume (gfx950) and the cleanup that follows from them: drop small components, keep
// the largest of a class, fill small enclosed holes.  A component is a maximal set of voxels of EQUAL value connected through
// face (6), face + edge (18) or face + edge + corner (26) neighbours, value 0 included, so one labelling serves every class and
// the background.  The id of a component is the linear index of its lowest-index voxel (its root): whatever order the unions
// happen in, the result is the same bits.  Exact integers throughout (utilities/components.py is the Python layer and the host
// route that gives the same integers).
//
// vs_label_components: block-based union-find, three launches, no grid-wide barrier, no host loop.
//  1 tile_kernel: one workgroup labels one tile of kTZ x kTY x kTX = 8 x 8 x 64 voxels in LDS.  A wave owns a row of 64 voxels
//    along x: one ballot of "differs from the voxel before" gives the runs, and every voxel starts with its run's first voxel as
//    parent - the x direction costs no union.  Runs are then united with the rows before them in y and z (and across the
//    diagonal offsets for 18 / 26) by LDS atomicMin unions; a pair is left out when a pair one voxel earlier in x already
//    joins the same two runs, so a union is issued about once per pair of touching runs, not once per voxel.  The tile is
//    flattened and written as GLOBAL indices: comp[v] = index of the lowest voxel of v's component within the tile.  The
//    workgroup also records whether the whole tile holds one value (workspace: one int32 per tile, the value or -1).
//  2 seam_kernel: one workgroup per tile unites across the tile's faces (edges and corners for 18 / 26) with global atomicMin
//    unions on comp.  Every pair of adjacent voxels in different tiles belongs to the later of the two voxels.  Two adjacent
//    tiles that each hold one value, the same one, are joined by ONE union of their first voxels (a tile of one value is one
//    component after launch 1) and none of their voxel pairs is looked at; a tile whose whole neighbourhood is like that reads
//    no label at all - the bulk of the background and of every large object.
//  3 flatten_kernel: comp[v] = root of v.
//  Parents only ever decrease (a root is linked below a smaller index, never the other way), so every find walks a strictly
//  decreasing chain and every union retry starts from a smaller index: all loops end on any input.  A find may read a parent
//  that another workgroup has already lowered; an older parent is still a voxel of the same component, and the atomicMin that
//  makes a link returns the truth, so stale reads cost a retry, never a wrong link.
//
// vs_component_sizes: size[root] = voxels, touches[root] = 1 when the component reaches a face of the volume.  A lane reads four
// consecutive ids; for each of the four voxel positions the lanes of a wave that hold the same id are grouped by ballots (up to
// eight ids per position, fewer once two of them were held by one lane only; the rest - small components - add on their own),
// and the group's first lane adds the group's count to a 32-entry cache in LDS that the wave keeps over its 32 steps across a
// contiguous span: an id leaves the cache, as ONE global atomic, when another id takes its slot or at the end.  A solid 512^3
// volume issues one atomic per wave, and the border between two big components costs cache hits, not same-address atomics.
// vs_component_largest: per label value the packed key (size << 32) | (0x7FFFFFFF - root), maximised in LDS, then globally.
// vs_components_apply: one sweep, every decision from the one labelling of the input.
#include "common.h"
#include "prof.h"

namespace {

constexpr int kTZ = 8, kTY = 8, kTX = 64;      // tile extents (utilities/components.py: TILE_Z / TILE_Y / TILE_X)
constexpr int kRows = kTZ * kTY;               // rows of one tile: 64
constexpr int kTile = kRows * kTX;             // 4096 voxels: 16 KiB of parents + 8 KiB of labels in LDS
constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kSpanSteps = 32;                 // vs_component_sizes: steps of 256 voxels a wave takes over its contiguous span
constexpr int64_t kLimit = 1LL << 31;

struct Grid {                                  // the volume and its tiling
    int Z, Y, X, nz, ny, nx;
};
Grid make_grid(int64_t Z, int64_t Y, int64_t X) {
    return Grid{(int)Z, (int)Y, (int)X, (int)((Z + kTZ - 1) / kTZ), (int)((Y + kTY - 1) / kTY), (int)((X + kTX - 1) / kTX)};
}

// ---- union-find --------------------------------------------------------------------------------------------------------------
// kScope: __HIP_MEMORY_SCOPE_WORKGROUP for the tile's LDS parents, __HIP_MEMORY_SCOPE_AGENT for comp in global memory
template <int kScope>
__device__ __forceinline__ int find_root(int* par, int a) {
    int p;
    while ((p = __hip_atomic_load(par + a, __ATOMIC_RELAXED, kScope)) != a) a = p;      // p < a: ends
    return a;
}

template <int kScope>
__device__ __forceinline__ void unite(int* par, int a, int b) {
    for (;;) {
        a = find_root<kScope>(par, a);
        b = find_root<kScope>(par, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = __hip_atomic_fetch_min(par + a, b, __ATOMIC_RELAXED, kScope);   // link the larger root below the smaller
        if (old == a) return;                    // a was a root: linked
        a = old;                                 // a had been linked below `old` (< a) meanwhile: join that with b as well
    }
}

// how many of the three offsets may be non-zero
__device__ __forceinline__ int reach_of(int connectivity) { return connectivity == 6 ? 1 : connectivity == 18 ? 2 : 3; }

// Whether the pair (voxel at x, its neighbour one row / plane earlier at x + dx) needs a union of its own.  c = the voxel's
// value (the neighbour's equals it), l / r = the values beside the voxel at x - 1 / x + 1, um / u0 = the values in the
// neighbour's row at x - 1 / x; a value that does not exist is negative.
//  dx = 0: not when the pair one voxel earlier joins the same two runs (l == c and um == c).
//  dx = +-1: not when the straight pair at x exists (u0 == c: the neighbour's row continues the run to x + dx), nor when the voxel's
//  own run continues to x + dx (side == c: the straight pair there exists).
__device__ __forceinline__ bool straight_pair_needed(int c, int l, int um) { return !(l == c && um == c); }
__device__ __forceinline__ bool diagonal_pair_needed(int c, int u0, int side) { return u0 != c && side != c; }

// ---- launch 1: tiles -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void tile_kernel(const uint8_t* __restrict__ labels, Grid g, int connectivity, int* __restrict__ comp,
                                                      int* __restrict__ tile_value) {
    __shared__ int par[kTile];
    __shared__ int16_t lab[kTile];             // the value, -1 outside the volume
    __shared__ int mixed;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int t = blockIdx.x;
    const int bx = t % g.nx; t /= g.nx;
    const int by = t % g.ny, bz = t / g.ny;
    const int z0 = bz * kTZ, y0 = by * kTY, x0 = bx * kTX;
    if (threadIdx.x == 0) mixed = 0;
    const int first = labels[((int64_t)z0 * g.Y + y0) * g.X + x0];      // the tile's first voxel is inside the volume
    __syncthreads();

    for (int r = wave; r < kRows; r += kWaves) {                          // uniform over the wave
        const int z = z0 + r / kTY, y = y0 + r % kTY, x = x0 + lane;
        const bool valid = z < g.Z && y < g.Y && x < g.X;
        const int v = valid ? (int)labels[((int64_t)z * g.Y + y) * g.X + x] : -1;
        const int left = __shfl_up(v, 1, 64);
        const uint64_t starts = __ballot(valid && (lane == 0 || left != v));
        const uint64_t upto = starts & (((uint64_t)2 << lane) - 1);      // lane 63: 2 << 63 wraps to 0, minus 1 = every bit
        lab[r * kTX + lane] = (int16_t)v;
        par[r * kTX + lane] = r * kTX + (valid ? 63 - __clzll((unsigned long long)upto) : lane);
        if (valid && v != first) mixed = 1;
    }
    __syncthreads();

    const int reach = reach_of(connectivity);
    for (int r = wave; r < kRows; r += kWaves) {
        const int tz = r / kTY, ty = r % kTY, idx = r * kTX + lane;
        const int c = lab[idx];
        if (c < 0) continue;
        const int l = lane > 0 ? (int)lab[idx - 1] : -1, rt = lane < 63 ? (int)lab[idx + 1] : -1;
#pragma unroll
        for (int k = 0; k < 4; ++k) {                                      // the four rows before this one: (dz, dy)
            const int dz = k == 0 ? 0 : -1, dy = k == 0 ? -1 : k - 2;
            const int nzero = (dz != 0) + (dy != 0);
            if (nzero > reach || tz + dz < 0 || ty + dy < 0 || ty + dy >= kTY) continue;
            const int nb = ((tz + dz) * kTY + ty + dy) * kTX + lane;
            const int u0 = lab[nb], um = lane > 0 ? (int)lab[nb - 1] : -1, up = lane < 63 ? (int)lab[nb + 1] : -1;
            if (u0 == c && straight_pair_needed(c, l, um)) unite<__HIP_MEMORY_SCOPE_WORKGROUP>(par, idx, nb);
            if (nzero < reach) {
                if (um == c && diagonal_pair_needed(c, u0, l)) unite<__HIP_MEMORY_SCOPE_WORKGROUP>(par, idx, nb - 1);
                if (up == c && diagonal_pair_needed(c, u0, rt)) unite<__HIP_MEMORY_SCOPE_WORKGROUP>(par, idx, nb + 1);
            }
        }
    }
    __syncthreads();

    for (int r = wave; r < kRows; r += kWaves) {
        const int z = z0 + r / kTY, y = y0 + r % kTY, x = x0 + lane;
        if (z >= g.Z || y >= g.Y || x >= g.X) continue;
        const int root = find_root<__HIP_MEMORY_SCOPE_WORKGROUP>(par, r * kTX + lane);
        const int rr = root / kTX;
        comp[((int64_t)z * g.Y + y) * g.X + x] = (int)(((int64_t)(z0 + rr / kTY) * g.Y + (y0 + rr % kTY)) * g.X + x0 + root % kTX);
    }
    if (threadIdx.x == 0) tile_value[blockIdx.x] = mixed ? -1 : first;
}

// ---- launch 2: seams -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int value_at(const uint8_t* __restrict__ labels, const Grid& g, int z, int y, int x) {
    return (z < 0 || y < 0 || x < 0 || z >= g.Z || y >= g.Y || x >= g.X) ? -1 : (int)labels[((int64_t)z * g.Y + y) * g.X + x];
}

__global__ __launch_bounds__(kThreads) void seam_kernel(const uint8_t* __restrict__ labels, Grid g, int connectivity, int* comp,
                                                      const int* __restrict__ tile_value) {
    __shared__ int near[27];                   // the values of the 27 tiles around this one ((sz + 1) * 9 + (sy + 1) * 3 + sx + 1); -2: no tile
    __shared__ int quiet;                      // this tile and every tile it touches hold one value, the same one
    int t = blockIdx.x;
    const int bx = t % g.nx; t /= g.nx;
    const int by = t % g.ny, bz = t / g.ny;
    const int z0 = bz * kTZ, y0 = by * kTY, x0 = bx * kTX;
    const int reach = reach_of(connectivity);
    if (threadIdx.x < 27) {
        const int sz = (int)threadIdx.x / 9 - 1, sy = ((int)threadIdx.x / 3) % 3 - 1, sx = (int)threadIdx.x % 3 - 1;
        const int nbz = bz + sz, nby = by + sy, nbx = bx + sx;
        const bool exists = nbz >= 0 && nby >= 0 && nbx >= 0 && nbz < g.nz && nby < g.ny && nbx < g.nx;
        near[threadIdx.x] = exists ? tile_value[((int64_t)nbz * g.ny + nby) * g.nx + nbx] : -2;
    }
    __syncthreads();
    const int me = near[13];
    if (threadIdx.x < 27) {
        const int sz = (int)threadIdx.x / 9 - 1, sy = ((int)threadIdx.x / 3) % 3 - 1, sx = (int)threadIdx.x % 3 - 1;
        const int nzero = (sz != 0) + (sy != 0) + (sx != 0);
        const int other = near[threadIdx.x];
        // one union for two whole tiles of one value: this tile's first voxel with the first voxel of the tile before it
        if (threadIdx.x < 13 && nzero <= reach && me >= 0 && other == me)
            unite<__HIP_MEMORY_SCOPE_AGENT>(comp, (int)(((int64_t)z0 * g.Y + y0) * g.X + x0),
                                            (int)(((int64_t)(z0 + sz * kTZ) * g.Y + (y0 + sy * kTY)) * g.X + x0 + sx * kTX));
        const bool same = me >= 0 && (other == me || other == -2 || nzero > reach);
        const uint64_t all = __ballot(same);                              // threads 0..26 sit in wave 0
        if (threadIdx.x == 0) quiet = (all & 0x7FFFFFFull) == 0x7FFFFFFull;
    }
    __syncthreads();
    if (quiet) return;

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int r = wave; r < kRows; r += kWaves) {
        const int tz = r / kTY, ty = r % kTY;
        const int z = z0 + tz, y = y0 + ty, x = x0 + lane;
        if (z >= g.Z || y >= g.Y || x >= g.X) continue;
        if (tz > 0 && ty > 0 && ty < kTY - 1 && lane > 0 && lane < kTX - 1) continue;    // every neighbour before it is in this tile
        const int64_t v = ((int64_t)z * g.Y + y) * g.X + x;
        const int c = labels[v];
        const int l = value_at(labels, g, z, y, x - 1);
        // the pair along x across the tile's face; left out when the row above joins the same two runs inside both tiles
        if (lane == 0 && l == c && !(me >= 0 && near[12] == me)) {
            if (!(ty > 0 && value_at(labels, g, z, y - 1, x) == c && value_at(labels, g, z, y - 1, x - 1) == c))
                unite<__HIP_MEMORY_SCOPE_AGENT>(comp, (int)v, (int)v - 1);
        }
        for (int k = 0; k < 4; ++k) {
            const int dz = k == 0 ? 0 : -1, dy = k == 0 ? -1 : k - 2;
            const int nzero = (dz != 0) + (dy != 0);
            const int nz_ = z + dz, ny_ = y + dy;
            if (nzero > reach || nz_ < 0 || ny_ < 0 || ny_ >= g.Y) continue;
            const int sz = tz + dz < 0 ? -1 : 0, sy = ty + dy < 0 ? -1 : ty + dy >= kTY ? 1 : 0;
            const int64_t nb = ((int64_t)nz_ * g.Y + ny_) * g.X + x;
            for (int dx = -1; dx <= 1; ++dx) {
                if (dx != 0 && nzero >= reach) continue;
                const int sx = lane + dx < 0 ? -1 : lane + dx >= kTX ? 1 : 0;
                if (sz == 0 && sy == 0 && sx == 0) continue;              // inside the tile: launch 1 joined it
                if (x + dx < 0 || x + dx >= g.X) continue;
                if (me >= 0 && near[(sz + 1) * 9 + (sy + 1) * 3 + sx + 1] == me) continue;    // two tiles of one value: joined above
                if ((int)labels[nb + dx] != c) continue;
                bool needed;
                if (dx == 0) needed = straight_pair_needed(c, l, value_at(labels, g, nz_, ny_, x - 1));
                else needed = diagonal_pair_needed(c, (int)labels[nb], value_at(labels, g, z, y, x + dx));
                if (needed) unite<__HIP_MEMORY_SCOPE_AGENT>(comp, (int)v, (int)(nb + dx));
            }
        }
    }
}

// ---- launch 3: flatten ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void flatten_kernel(int* comp, int64_t n) {
    for (int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x; v < n; v += (int64_t)gridDim.x * kThreads) {
        const int p = comp[v];
        if (p == (int)v) continue;
        const int root = find_root<__HIP_MEMORY_SCOPE_AGENT>(comp, p);
        if (root != p) comp[v] = root;          // another lane may read comp[v] meanwhile: the old parent and the root are both on its chain
    }
}

// ---- sizes ---------------------------------------------------------------------------------------------------------------------
constexpr int kCacheSlots = 32;                // per wave: (id, pending count, pending touch) of the ids the wave keeps meeting
constexpr int kRounds = 8;                     // ids per voxel position a wave groups by ballot (fewer once two groups were single lanes)

__device__ __forceinline__ void flush_entry(int* size, uint8_t* touches, int key, int count, int touch) {
    if (key >= 0 && count > 0) {
        atomicAdd(size + key, count);
        if (touch && touches) touches[key] = 1;
    }
}

__global__ __launch_bounds__(kThreads) void sizes_kernel(const int* __restrict__ comp, Grid g, int64_t n, int* __restrict__ size,
                                                       uint8_t* __restrict__ touches) {
    // one lane at a time (the leader of a group) touches its wave's cache, in program order: volatile keeps the order
    __shared__ volatile int cache_key[kWaves][kCacheSlots], cache_count[kWaves][kCacheSlots], cache_touch[kWaves][kCacheSlots];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane < kCacheSlots) { cache_key[wave][lane] = -1; cache_count[wave][lane] = 0; cache_touch[wave][lane] = 0; }
    const int64_t span = (int64_t)kSpanSteps * 256;
    const int64_t base = ((int64_t)blockIdx.x * kWaves + wave) * span;
    for (int step = 0; step < kSpanSteps; ++step) {
        if (base + (int64_t)step * 256 >= n) break;                       // uniform over the wave
        const int64_t v0 = base + (int64_t)step * 256 + lane * 4;
        int id[4] = {-1, -1, -1, -1};
        if (v0 + 4 <= n) {
            const int4 q = *reinterpret_cast<const int4*>(comp + v0);
            id[0] = q.x; id[1] = q.y; id[2] = q.z; id[3] = q.w;
        } else {
            for (int j = 0; j < 4; ++j)
                if (v0 + j < n) id[j] = comp[v0 + j];
        }
        uint32_t face = 0;                      // bit j: voxel j lies on a face of the volume
        if (v0 < n) {
            int x = (int)(v0 % g.X);
            const int64_t row = v0 / g.X;
            int y = (int)(row % g.Y), z = (int)(row / g.Y);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool f = (g.X > 1 && (x == 0 || x == g.X - 1)) || (g.Y > 1 && (y == 0 || y == g.Y - 1)) || (g.Z > 1 && (z == 0 || z == g.Z - 1));
                face |= (uint32_t)f << j;
                if (++x == g.X) { x = 0; if (++y == g.Y) { y = 0; ++z; } }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {            // voxel j of every lane: the lanes that hold one id add once, through their first lane
            const bool has = id[j] >= 0, onface = (face >> j) & 1u;
            uint64_t rest = __ballot(has);
            const uint64_t faces = __ballot(has && onface);
            for (int round = 0, alone = 0; round < kRounds && alone < 2 && rest; ++round) {      // uniform over the wave
                const int leader = __ffsll((unsigned long long)rest) - 1;
                const int key = __shfl(id[j], leader, 64);
                const uint64_t same = __ballot(has && id[j] == key);
                alone += (same & (same - 1)) == 0;                        // a second group of one lane: the rest are small components too
                if (lane == leader) {
                    int slot = (int)(((uint32_t)key * 2654435761u) >> 27);               // two ways: the slot and its neighbour
                    if (cache_key[wave][slot] != key && (cache_key[wave][slot ^ 1] == key || cache_key[wave][slot ^ 1] < 0)) slot ^= 1;
                    const int touch = (faces & same) != 0;
                    if (cache_key[wave][slot] == key) {
                        cache_count[wave][slot] += __popcll(same);
                        cache_touch[wave][slot] |= touch;
                    } else {
                        flush_entry(size, touches, cache_key[wave][slot], cache_count[wave][slot], cache_touch[wave][slot]);
                        cache_key[wave][slot] = key; cache_count[wave][slot] = __popcll(same); cache_touch[wave][slot] = touch;
                    }
                }
                rest &= ~same;
            }
            if ((rest >> lane) & 1) {            // more than kRounds ids among the 64 voxels: small components, spread addresses
                atomicAdd(size + id[j], 1);
                if (onface && touches) touches[id[j]] = 1;
            }
        }
    }
    if (lane < kCacheSlots) flush_entry(size, touches, cache_key[wave][lane], cache_count[wave][lane], cache_touch[wave][lane]);
}

// ---- largest -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void largest_kernel(const uint8_t* __restrict__ labels, const int* __restrict__ size, int64_t n,
                                                         unsigned long long* __restrict__ keys) {
    __shared__ unsigned long long best[256];
    best[threadIdx.x] = 0;
    __syncthreads();
    for (int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x; v < n; v += (int64_t)gridDim.x * kThreads) {
        const int s = size[v];
        if (s > 0) atomicMax(&best[labels[v]], ((unsigned long long)(uint32_t)s << 32) | (unsigned long long)(0x7FFFFFFF - (int)v));
    }
    __syncthreads();
    if (best[threadIdx.x]) atomicMax(keys + threadIdx.x, best[threadIdx.x]);
}

// ---- apply ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void apply_kernel(const uint8_t* __restrict__ labels, const int* __restrict__ comp,
                                                       const int* __restrict__ size, const uint8_t* __restrict__ touches,
                                                       const int* __restrict__ min_size, const int* __restrict__ keep_root, int background,
                                                       int hole_max, uint8_t* __restrict__ out, unsigned long long* __restrict__ counts, int64_t n) {
    __shared__ int min_of[256], keep_of[256];
    __shared__ unsigned long long total[4];
    min_of[threadIdx.x] = min_size[threadIdx.x];
    keep_of[threadIdx.x] = keep_root[threadIdx.x];
    if (threadIdx.x < 4) total[threadIdx.x] = 0;
    __syncthreads();
    // whether the component (value c != background, root r) is cleared
    auto cleared = [&](int c, int r) { return size[r] < min_of[c] || (keep_of[c] >= 0 && r != keep_of[c]); };
    uint32_t mine[4] = {0u, 0u, 0u, 0u};        // cleared components, cleared voxels, filled holes, filled voxels (< 2^31 each)
    int last_root = -1, last_out = 0;           // consecutive voxels mostly share a component: decide once
    bool last_cleared = false, last_filled = false;
    auto decide = [&](int64_t v, int c, int r) -> uint32_t {
        if (r != last_root) {
            last_root = r;
            last_out = c;
            last_cleared = last_filled = false;
            if (c != background) {
                last_cleared = cleared(c, r);
                if (last_cleared) last_out = background;
            } else if (hole_max > 0 && r > 0 && size[r] <= hole_max && touches[r] == 0) {
                const int c2 = labels[r - 1];    // the voxel in front of the root: another value, so not background
                last_out = (c2 == background || cleared(c2, comp[r - 1])) ? background : c2;
                last_filled = last_out != background;
            }
        }
        mine[1] += last_cleared;
        mine[3] += last_filled;
        mine[0] += last_cleared && r == (int)v;
        mine[2] += last_filled && r == (int)v;
        return (uint32_t)last_out;
    };
    const int64_t nq = n >> 2;                  // four voxels per lane: one word of labels, one vector of ids, one word stored
    for (int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x; q < nq; q += (int64_t)gridDim.x * kThreads) {
        const uint32_t w = reinterpret_cast<const uint32_t*>(labels)[q];
        const int4 id = reinterpret_cast<const int4*>(comp)[q];
        uint32_t o = decide(4 * q, w & 0xff, id.x);
        o |= decide(4 * q + 1, (w >> 8) & 0xff, id.y) << 8;
        o |= decide(4 * q + 2, (w >> 16) & 0xff, id.z) << 16;
        o |= decide(4 * q + 3, w >> 24, id.w) << 24;
        reinterpret_cast<uint32_t*>(out)[q] = o;
    }
    if (blockIdx.x == 0 && threadIdx.x < (int)(n & 3)) {
        const int64_t v = (nq << 2) + threadIdx.x;
        out[v] = (uint8_t)decide(v, labels[v], comp[v]);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint32_t s = mine[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
        if ((threadIdx.x & 63) == 0 && s) atomicAdd(&total[k], (unsigned long long)s);
    }
    __syncthreads();
    if (threadIdx.x < 4 && total[threadIdx.x]) atomicAdd(counts + threadIdx.x, total[threadIdx.x]);
}

int64_t sweep_grid(int64_t n) {
    int64_t grid = (n + kThreads - 1) / kThreads;
    if (grid > persistent_workgroups()) grid = persistent_workgroups();
    return grid < 1 ? 1 : grid;
}

}  // namespace

#define VS_COMPONENT_EXTENTS(what)                                                                                                         \
    VS_REQUIRE(extents_fit(Z, Y, X, 0), what ": extents %lld x %lld x %lld - every extent must be at least 1 and the volume below 2^31 voxels " \
               "(component ids are int32 voxel indices)", (long long)Z, (long long)Y, (long long)X)

extern "C" size_t vs_components_workspace_bytes(int64_t Z, int64_t Y, int64_t X) {
    if (!extents_fit(Z, Y, X, 0)) return 0;
    const Grid g = make_grid(Z, Y, X);
    return (size_t)g.nz * g.ny * g.nx * sizeof(int);
}

extern "C" int vs_label_components(const uint8_t* labels, int64_t Z, int64_t Y, int64_t X, int connectivity, int32_t* comp, void* workspace,
                                   size_t workspace_bytes, void* stream) {
    VS_COMPONENT_EXTENTS("label_components");
    VS_REQUIRE(connectivity == 6 || connectivity == 18 || connectivity == 26, "label_components: connectivity %d - it is 6, 18 or 26", connectivity);
    VS_REQUIRE(labels && comp, "label_components: null volume");
    const size_t need = vs_components_workspace_bytes(Z, Y, X);
    VS_REQUIRE(workspace && workspace_bytes >= need, "label_components: workspace of %zu bytes, %zu needed (vs_components_workspace_bytes)",
               workspace ? workspace_bytes : (size_t)0, need);
    VS_REQUIRE((uintptr_t)comp % 4 == 0 && (uintptr_t)workspace % 4 == 0, "label_components: comp and workspace must be 4-byte aligned");
    const Grid g = make_grid(Z, Y, X);
    const int64_t tiles = (int64_t)g.nz * g.ny * g.nx, n = Z * Y * X;      // tiles <= n < 2^31
    hipStream_t s = (hipStream_t)stream;
    int* tile_value = (int*)workspace;
    const double volume = (double)n;           // profile records (tools/components_probe.py): tiles, seams, flatten, in launch order
    {
        ProfScope prof(PK_POOL_MISC, 0.0, 5.0 * volume, s);              // labels read, ids written
        hipLaunchKernelGGL(tile_kernel, dim3((unsigned)tiles), dim3(kThreads), 0, s, labels, g, connectivity, comp, tile_value);
        VS_LAUNCH_CHECK();
    }
    {
        ProfScope prof(PK_POOL_MISC, 0.0, 0.0, s);                       // the faces of the tiles that are not of one value
        hipLaunchKernelGGL(seam_kernel, dim3((unsigned)tiles), dim3(kThreads), 0, s, labels, g, connectivity, comp, tile_value);
        VS_LAUNCH_CHECK();
    }
    {
        ProfScope prof(PK_POOL_MISC, 0.0, 8.0 * volume, s);              // ids read and written
        hipLaunchKernelGGL(flatten_kernel, dim3((unsigned)sweep_grid(n)), dim3(kThreads), 0, s, comp, n);
        VS_LAUNCH_CHECK();
    }
    return VS_OK;
}

extern "C" int vs_component_sizes(const int32_t* comp, int64_t Z, int64_t Y, int64_t X, int32_t* size, uint8_t* touches, void* stream) {
    VS_COMPONENT_EXTENTS("component_sizes");
    VS_REQUIRE(comp && size, "component_sizes: null argument");
    VS_REQUIRE((uintptr_t)comp % 16 == 0 && (uintptr_t)size % 4 == 0, "component_sizes: comp must be 16-byte, size 4-byte aligned");
    const int64_t n = Z * Y * X;
    hipStream_t s = (hipStream_t)stream;
    VS_CHECK_HIP(hipMemsetAsync(size, 0, (size_t)n * sizeof(int32_t), s));
    if (touches) VS_CHECK_HIP(hipMemsetAsync(touches, 0, (size_t)n, s));
    const int64_t per_wg = (int64_t)kWaves * kSpanSteps * 256;
    ProfScope prof(PK_POOL_MISC, 0.0, 4.0 * (double)n, s);
    hipLaunchKernelGGL(sizes_kernel, dim3((unsigned)((n + per_wg - 1) / per_wg)), dim3(kThreads), 0, s, comp, make_grid(Z, Y, X), n, size, touches);
    VS_LAUNCH_CHECK();
    return VS_OK;
}

extern "C" int vs_component_largest(const uint8_t* labels, const int32_t* size, int64_t n, int64_t* key_per_value, void* stream) {
    VS_REQUIRE(labels && size && key_per_value, "component_largest: null argument");
    VS_REQUIRE(n >= 1 && n < kLimit, "component_largest: %lld voxels - the volume must hold at least 1 and fewer than 2^31", (long long)n);
    VS_REQUIRE((uintptr_t)size % 4 == 0 && (uintptr_t)key_per_value % 8 == 0, "component_largest: size must be 4-byte, the keys 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    VS_CHECK_HIP(hipMemsetAsync(key_per_value, 0, 256 * sizeof(int64_t), s));
    ProfScope prof(PK_POOL_MISC, 0.0, 4.0 * (double)n, s);
    hipLaunchKernelGGL(largest_kernel, dim3((unsigned)sweep_grid(n)), dim3(kThreads), 0, s, labels, size, n, (unsigned long long*)key_per_value);
    VS_LAUNCH_CHECK();
    return VS_OK;
}

extern "C" int vs_components_apply(const uint8_t* labels, const int32_t* comp, const int32_t* size, const uint8_t* touches, const int32_t* min_size,
                                   const int32_t* keep_root, int background, int64_t hole_max, int64_t n, uint8_t* out, int64_t* counts,
                                   void* stream) {
    VS_REQUIRE(labels && comp && size && min_size && keep_root && out && counts, "components_apply: null argument");
    VS_REQUIRE(n >= 1 && n < kLimit, "components_apply: %lld voxels - the volume must hold at least 1 and fewer than 2^31", (long long)n);
    VS_REQUIRE(background >= 0 && background <= 255, "components_apply: background %d is not a uint8 value", background);
    VS_REQUIRE(hole_max <= 0 || touches, "components_apply: filling holes needs the touches flags of vs_component_sizes");
    VS_REQUIRE(out + n <= labels || labels + n <= out, "components_apply: out must not overlap labels (a hole reads the voxel in front of its root)");
    VS_REQUIRE((uintptr_t)comp % 16 == 0 && ((uintptr_t)labels | (uintptr_t)out | (uintptr_t)size | (uintptr_t)min_size | (uintptr_t)keep_root) % 4 == 0 &&
               (uintptr_t)counts % 8 == 0, "components_apply: comp must be 16-byte, labels / out / the int32 arguments 4-byte, counts 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    VS_CHECK_HIP(hipMemsetAsync(counts, 0, 4 * sizeof(int64_t), s));
    ProfScope prof(PK_POOL_MISC, 0.0, 6.0 * (double)n, s);
    hipLaunchKernelGGL(apply_kernel, dim3((unsigned)sweep_grid(n)), dim3(kThreads), 0, s, labels, comp, size, touches, min_size, keep_root, background,
                       (int)(hole_max > 0x7FFFFFFF ? 0x7FFFFFFF : hole_max < 0 ? 0 : hole_max), out, (unsigned long long*)counts, n);
    VS_LAUNCH_CHECK();
    return VS_OK;
}
