// Per-component measurements of a uint8 label volume (gfx950): from the labels and the roots of vs_label_components, one sweep
// fills a table of kFields = 20 exact int64 figures per measured component - voxels, the first and second moments of the
// coordinates, the bounding box, the exposed faces across each axis and whether the component touches the volume's boundary
// (include/volseg_hip.h lists the fields; utilities/measurements.py is the Python layer, the derived figures and the host route
// that gives the same integers).  Integer adds, minima and maxima commute: atomics are allowed and the table is the same bits on
// every run.  What the kernel has to get right is contention - the background and every large object put millions of voxels
// into ONE row of 20 accumulators - so a global atomic is issued per wave and id, never per voxel.
//
// vs_component_moments: two launches (the table's initial values, then the sweep), no grid-wide barrier, no host loop.
//  * A wave owns a contiguous span of kSpanSteps x 256 voxels of the flattened volume.  Per step a lane reads one 4-byte word of
//    labels and, with the same width, the words at -X, +X, -XY, +XY (the four neighbouring rows; a scalar path where those
//    addresses are not 4-byte aligned or leave the volume); shuffles then hand lane l the voxel 64 k + l of the step, k = 0 .. 3,
//    so that the 64 lanes of a sub-step hold 64 consecutive voxels.
//  * Runs along x.  Face-adjacent voxels of equal value share a component under 6, 18 and 26, so "the value differs from the
//    lane before" (or the row starts, or the sub-step starts) gives the runs in one ballot and no id is read for it.  Only a
//    run's first lane goes on: it reads comp at the run's first voxel and row_of_root at that root - one lookup per run - and a
//    run whose row is -1 costs nothing further (64 voxels without a measured run are left before any neighbour is compared).
//    A run [x0, x1] at (z, y) of length L contributes closed forms: L, L z, L y, sum x = L (x0 + x1) / 2, L z^2, L y^2,
//    sum x^2 = S2(x1) - S2(x0 - 1) with S2(n) = n (n + 1) (2 n + 1) / 6 (divided before the last product, so nothing exceeds
//    the result), L z y, z sum x, y sum x, and its ends as the x bounds.
//  * Exposed faces are per-voxel comparisons with the six neighbours (outside the volume counts as another value; an axis of
//    length 1 has no faces).  Six ballots, and a seventh for "on the boundary", are masked with the run's lanes and popcounted, so
//    they enter as per-run figures too.  A run cut by the sub-step's edge compares with the true neighbour beyond it.
//  * The runs of a sub-step are grouped by table row with ballots, kRounds rows at most; the group's first lane claims a slot
//    of a wave-private cache in LDS (kSlots rows of 20 int64, two ways) and the group's lanes add into it with LDS atomics -
//    or, where the group has several runs and the 64 voxels lie in one row of the volume, the first lane alone adds the figures
//    of the whole group, which follow from the mask of the group's voxels by popcounts (group_figures): big objects that
//    interleave voxel by voxel would otherwise meet, a dozen lanes at a time, on the same 20 LDS addresses.  A
//    row leaves the cache - 20 lanes, one 64-bit global atomicAdd / atomicMin / atomicMax each, zeros and identities left out -
//    when another row takes its slot and at the end of the span.  Runs left after the rounds belong to small components: they
//    go straight to global atomics on addresses that are spread.
//  A volume of one value issues at most 20 global atomics per wave (one wave per 8192 voxels), and so does the border between two
//  big objects; random labels with every crumb measured pay one eviction per run, which is what they would pay without a cache.
//
// vs_object_moments: the same sweep for ANY labelling whose ids are member voxel indices (the separated objects of
// utilities/separation.py): a run is a stretch of equal ID and an exposed face a face neighbour with another id, so two objects of
// one value that touch count their contact as surface.  It is the second instantiation of the one kernel - the policy (ByValue /
// ById) says what a run and a neighbour are compared by and how four elements are loaded (one 4-byte word / one 16-byte vector per
// lane and neighbouring row); everything after the ballots is shared.  On a component labelling the two give the same bits:
// components of one value are never face-adjacent.
#include <limits.h>

#include "common.h"
#include "prof.h"

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kSpanSteps = 32;                 // steps of 256 voxels a wave takes over its contiguous span
constexpr int kSlots = 32;                     // rows a wave's cache holds
constexpr int kRounds = 8;                     // rows per sub-step a wave groups by ballot
constexpr int kFields = 20;                    // utilities/measurements.py FIELDS

// fields 10, 12, 14 are minima, 11, 13, 15 and 19 maxima (19: 0 / 1), the others sums
__device__ __forceinline__ bool is_min(int f) { return f == 10 || f == 12 || f == 14; }
__device__ __forceinline__ bool is_max(int f) { return f == 11 || f == 13 || f == 15 || f == 19; }
__device__ __forceinline__ long long identity(int f) { return is_min(f) ? LLONG_MAX : (is_max(f) && f != 19) ? -1 : 0; }

// v into the table: identities issue nothing
__device__ __forceinline__ void merge_global(long long* p, int f, long long v) {
    if (is_min(f)) {
        if (v != LLONG_MAX) atomicMin(p, v);
    } else if (is_max(f)) {
        if (v > identity(f)) atomicMax(p, v);
    } else if (v) {
        atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);
    }
}

// v into a slot of the wave's cache: the lanes of a group meet on one address
__device__ __forceinline__ void merge_lds(long long* p, int f, long long v) {
    if (is_min(f)) __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else if (is_max(f)) __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else if (v) __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// the wave's LDS accesses stay in program order: the leader's claim, the group's adds, a flush's reads
__device__ __forceinline__ void cache_fence() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); }

// a cached row leaves: lane f carries field f, the slot is left holding identities
__device__ __forceinline__ void flush_slot(long long* __restrict__ table, long long* slot_val, int row, int lane) {
    if (lane < kFields) {
        merge_global(table + (int64_t)row * kFields + lane, lane, slot_val[lane]);
        slot_val[lane] = identity(lane);
    }
}

// What delimits a run and what a neighbour is compared by is the sweep's policy; the wave cache, the closed forms and the group
// figures are shared.  A policy loads the four elements src[a .. a + 3] as one word (anything for an element outside the volume:
// the sweep asks for the coordinate first), hands lane l of sub-step k element 64 k + l of the step - element l % 4 of the word
// that lane 16 k + l / 4 loaded - and names the component of a run from its first voxel.
struct ByValue {                               // vs_component_moments: runs and faces from the label VALUE, the id read once per run
    using Elem = uint8_t;
    using Word = uint32_t;
    static __device__ __forceinline__ Word load(const Elem* __restrict__ labels, int64_t a, int64_t n, bool aligned) {
        if (aligned && a >= 0 && a + 4 <= n) return *reinterpret_cast<const uint32_t*>(labels + a);
        uint32_t w = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (a + j >= 0 && a + j < n) w |= (uint32_t)labels[a + j] << (8 * j);
        return w;
    }
    static __device__ __forceinline__ Word none() { return 0u; }
    static __device__ __forceinline__ int pick(Word w, int k, int lane) {
        return (int)(((uint32_t)__shfl((int)w, 16 * k + (lane >> 2), 64) >> (8 * (lane & 3))) & 0xffu);
    }
    static __device__ __forceinline__ int id_of(const int* __restrict__ comp, int64_t p, int) { return comp[p]; }
};

struct ById {                                  // vs_object_moments: runs and faces from the object ID itself, 16 bytes per lane and load
    using Elem = int;
    using Word = int4;
    static __device__ __forceinline__ Word load(const Elem* __restrict__ ids, int64_t a, int64_t n, bool aligned) {
        if (aligned && a >= 0 && a + 4 <= n) return *reinterpret_cast<const int4*>(ids + a);
        int e[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) e[j] = a + j >= 0 && a + j < n ? ids[a + j] : -1;
        return make_int4(e[0], e[1], e[2], e[3]);
    }
    static __device__ __forceinline__ Word none() { return make_int4(-1, -1, -1, -1); }
    static __device__ __forceinline__ int pick(Word w, int k, int lane) {
        const int src = 16 * k + (lane >> 2), sel = lane & 3;
        const int x = __shfl(w.x, src, 64), y = __shfl(w.y, src, 64), z = __shfl(w.z, src, 64), t = __shfl(w.w, src, 64);
        return sel == 0 ? x : sel == 1 ? y : sel == 2 ? z : t;
    }
    static __device__ __forceinline__ int id_of(const int* __restrict__, int64_t, int own) { return own; }
};

// sum of i^2 for i = 0 .. m, m >= -1; the division comes before the last product, so no intermediate exceeds the result
__device__ __forceinline__ long long sum_squares(long long m) {
    const long long t = m * (m + 1) / 2, u = 2 * m + 1;
    return t % 3 == 0 ? (t / 3) * u : t * (u / 3);
}

// The figures of a whole group at once, where every voxel of the sub-step lies in one row (z, y) and lane l holds x = xb + l: from
// the mask of the group's voxels, sum l = sum over bits b of 2^b popcount(mask & B_b) and sum l^2 = sum over bits b, c of 2^(b + c)
// popcount(mask & B_b & B_c), with B_b the lanes whose index has bit b set.  The face ballots are masked alike.
__device__ __forceinline__ void group_figures(long long* f, uint64_t mask, long long xb, long long zz, long long yy, uint64_t bz0, uint64_t bz1,
                                              uint64_t by0, uint64_t by1, uint64_t bx0, uint64_t bx1, uint64_t bt) {
    constexpr uint64_t kBit[6] = {0xAAAAAAAAAAAAAAAAull, 0xCCCCCCCCCCCCCCCCull, 0xF0F0F0F0F0F0F0F0ull,
                                  0xFF00FF00FF00FF00ull, 0xFFFF0000FFFF0000ull, 0xFFFFFFFF00000000ull};
    const long long L = __popcll(mask);
    long long s1 = 0, s2 = 0;
#pragma unroll
    for (int b = 0; b < 6; ++b) {
        const uint64_t mb = mask & kBit[b];
        s1 += (long long)__popcll(mb) << b;
        s2 += (long long)__popcll(mb) << (2 * b);
#pragma unroll
        for (int c = b + 1; c < 6; ++c) s2 += (long long)__popcll(mb & kBit[c]) << (b + c + 1);
    }
    const long long sx = xb * L + s1;
    f[0] = L; f[1] = L * zz; f[2] = L * yy; f[3] = sx;
    f[4] = L * zz * zz; f[5] = L * yy * yy; f[6] = xb * xb * L + 2 * xb * s1 + s2;
    f[7] = L * zz * yy; f[8] = zz * sx; f[9] = yy * sx;
    f[10] = zz; f[11] = zz; f[12] = yy; f[13] = yy;
    f[14] = xb + __ffsll((unsigned long long)mask) - 1; f[15] = xb + 63 - __clzll((long long)mask);
    f[16] = __popcll(bz0 & mask) + __popcll(bz1 & mask);
    f[17] = __popcll(by0 & mask) + __popcll(by1 & mask);
    f[18] = __popcll(bx0 & mask) + __popcll(bx1 & mask);
    f[19] = (bt & mask) != 0;
}

__global__ __launch_bounds__(kThreads) void table_init_kernel(long long* __restrict__ table, int64_t entries, int Z, int Y, int X) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= entries) return;
    const int f = (int)(i % kFields);
    table[i] = f == 10 ? Z : f == 12 ? Y : f == 14 ? X : (f == 11 || f == 13 || f == 15) ? -1 : 0;      // an empty box: min = extent, max = -1
}

template <typename Policy>
__global__ __launch_bounds__(kThreads) void moments_kernel(const typename Policy::Elem* __restrict__ labels, const int* __restrict__ comp,
                                                         const int* __restrict__ row_of_root, int Z, int Y, int X, int64_t n, int rows,
                                                         long long* __restrict__ table) {
    __shared__ long long cache_val[kWaves][kSlots][kFields];
    __shared__ int cache_key[kWaves][kSlots];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long(*val)[kFields] = cache_val[wave];
    int* key = cache_key[wave];
    for (int i = lane; i < kSlots * kFields; i += 64) val[i / kFields][i % kFields] = identity(i % kFields);
    if (lane < kSlots) key[lane] = -1;
    cache_fence();

    const int64_t plane = (int64_t)Y * X;
    const bool word_y = X % 4 == 0, word_z = plane % 4 == 0;           // the neighbouring rows are aligned like the row itself
    const int64_t base = ((int64_t)blockIdx.x * kWaves + wave) * kSpanSteps * 256;
    for (int step = 0; step < kSpanSteps; ++step) {
        const int64_t sb = base + (int64_t)step * 256;
        if (sb >= n) break;                                             // uniform over the wave
        const int64_t v0 = sb + lane * 4;
        using Word = typename Policy::Word;
        const Word wc = Policy::load(labels, v0, n, true);
        const Word wy0 = Y > 1 ? Policy::load(labels, v0 - X, n, word_y) : Policy::none(), wy1 = Y > 1 ? Policy::load(labels, v0 + X, n, word_y) : Policy::none();
        const Word wz0 = Z > 1 ? Policy::load(labels, v0 - plane, n, word_z) : Policy::none(), wz1 = Z > 1 ? Policy::load(labels, v0 + plane, n, word_z) : Policy::none();
        const int before = sb > 0 ? (int)labels[sb - 1] : -1, after = sb + 256 < n ? (int)labels[sb + 256] : -1;      // beyond the step's ends
        int c[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int value = Policy::pick(wc, k, lane);                        // every lane shuffles: a lane beyond the volume may hold a word that is read
            c[k] = sb + 64 * k + lane < n ? value : -1;
        }

        // the runs of all four sub-steps and their rows first: the two dependent lookups (comp at a run's first voxel, row_of_root at
        // that root) of the four sub-steps are in flight together, not one pair after the other between the cache's fences
        int xs[4], lines[4], ids[4], rows_of[4];
        uint64_t starts_of[4], valids_of[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t p = sb + 64 * k + lane;
            const bool valid = p < n;
            const uint32_t pu = valid ? (uint32_t)p : 0u, line = pu / (uint32_t)X;
            xs[k] = (int)(pu - line * (uint32_t)X);
            lines[k] = (int)line;
            int left = __shfl_up(c[k], 1, 64);
            const int edge_l = k == 0 ? before : __shfl(c[k > 0 ? k - 1 : 0], 63, 64);
            if (lane == 0) left = edge_l;
            const bool start = valid && (lane == 0 || xs[k] == 0 || left != c[k]);
            starts_of[k] = __ballot(start);
            valids_of[k] = __ballot(valid);
            ids[k] = start ? Policy::id_of(comp, p, c[k]) : -1;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            rows_of[k] = ids[k] >= 0 && ids[k] < n ? row_of_root[ids[k]] : -1;         // once per run
            if (rows_of[k] >= rows) rows_of[k] = -1;
        }

#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (sb + 64 * k >= n) break;                                // uniform over the wave
            const int row = rows_of[k];
            uint64_t rest = __ballot(row >= 0);
            if (!rest) continue;                                        // uniform: 64 voxels nobody measures - most of a volume whose background is left out

            const bool valid = sb + 64 * k + lane < n;
            const uint64_t starts = starts_of[k], valids = valids_of[k];
            const int x = xs[k], y = (int)((uint32_t)lines[k] % (uint32_t)Y), z = (int)((uint32_t)lines[k] / (uint32_t)Y);
            const int cc = c[k];
            int left = __shfl_up(cc, 1, 64), right = __shfl_down(cc, 1, 64);
            const int edge_l = k == 0 ? before : __shfl(c[k > 0 ? k - 1 : 0], 63, 64);
            const int edge_r = k == 3 ? after : __shfl(c[k < 3 ? k + 1 : 3], 0, 64);
            if (lane == 0) left = edge_l;
            if (lane == 63) right = edge_r;

            const int ny0 = Policy::pick(wy0, k, lane), ny1 = Policy::pick(wy1, k, lane), nz0 = Policy::pick(wz0, k, lane), nz1 = Policy::pick(wz1, k, lane);
            const uint64_t bx0 = __ballot(valid && X > 1 && (x == 0 || left != cc)), bx1 = __ballot(valid && X > 1 && (x == X - 1 || right != cc));
            const uint64_t by0 = __ballot(valid && Y > 1 && (y == 0 || ny0 != cc)), by1 = __ballot(valid && Y > 1 && (y == Y - 1 || ny1 != cc));
            const uint64_t bz0 = __ballot(valid && Z > 1 && (z == 0 || nz0 != cc)), bz1 = __ballot(valid && Z > 1 && (z == Z - 1 || nz1 != cc));
            const uint64_t bt = __ballot(valid && ((X > 1 && (x == 0 || x == X - 1)) || (Y > 1 && (y == 0 || y == Y - 1)) || (Z > 1 && (z == 0 || z == Z - 1))));

            long long f[kFields];
#pragma unroll
            for (int i = 0; i < kFields; ++i) f[i] = 0;
            if (row >= 0) {
                const uint64_t upper = starts & ~(((uint64_t)2 << lane) - 1);                  // lane 63: 2 << 63 wraps to 0, minus 1 = every bit
                const int end = upper ? __ffsll((unsigned long long)upper) - 2 : __popcll(valids) - 1;      // valid lanes are a prefix
                const uint64_t mine = (((uint64_t)2 << end) - 1) & ~(((uint64_t)1 << lane) - 1);
                const long long L = end - lane + 1, zz = z, yy = y, x0 = x, x1 = x + L - 1;
                const long long sx = L * (x0 + x1) / 2;
                f[0] = L; f[1] = L * zz; f[2] = L * yy; f[3] = sx;
                f[4] = L * zz * zz; f[5] = L * yy * yy; f[6] = sum_squares(x1) - sum_squares(x0 - 1);
                f[7] = L * zz * yy; f[8] = zz * sx; f[9] = yy * sx;
                f[10] = zz; f[11] = zz; f[12] = yy; f[13] = yy; f[14] = x0; f[15] = x1;
                f[16] = __popcll(bz0 & mine) + __popcll(bz1 & mine);
                f[17] = __popcll(by0 & mine) + __popcll(by1 & mine);
                f[18] = __popcll(bx0 & mine) + __popcll(bx1 & mine);
                f[19] = (bt & mine) != 0;
            }

            const bool one_row = __shfl(x, 0, 64) + __popcll(valids) - 1 < X;                // uniform: no lane of the sub-step wraps to the next row
            for (int round = 0; round < kRounds && rest; ++round) {    // uniform over the wave
                const int leader = __ffsll((unsigned long long)rest) - 1;
                const int want = __shfl(row, leader, 64);
                const uint64_t same = __ballot(row == want);
                int slot = 0, evict = 0;
                if (lane == leader) {
                    slot = (int)(((uint32_t)want * 2654435761u) >> 27);                       // two ways: the slot and its neighbour
                    if (key[slot] != want && (key[slot ^ 1] == want || key[slot ^ 1] < 0)) slot ^= 1;
                    evict = key[slot] != want && key[slot] >= 0;
                }
                slot = __shfl(slot, leader, 64);
                evict = __shfl(evict, leader, 64);
                if (evict) flush_slot(table, val[slot], key[slot], lane);
                cache_fence();
                if (lane == leader) key[slot] = want;
                uint64_t adders = same;
                if (one_row && (same & (same - 1))) {                   // uniform: several runs of one row of voxels - their figures at once, one adder
                    const uint64_t upto = starts & (((uint64_t)2 << lane) - 1);
                    const int row_here = __shfl(row, valid ? 63 - __clzll((long long)upto) : lane, 64);       // the row of the run this lane's voxel is in
                    const uint64_t members = __ballot(valid && row_here == want);
                    if (lane == leader) group_figures(f, members, x - lane, z, y, bz0, bz1, by0, by1, bx0, bx1, bt);
                    adders = (uint64_t)1 << leader;
                }
                if ((adders >> lane) & 1) {
#pragma unroll
                    for (int i = 0; i < kFields; ++i) merge_lds(&val[slot][i], i, f[i]);
                }
                cache_fence();
                rest &= ~same;
            }
            if ((rest >> lane) & 1) {            // more than kRounds rows among the runs of 64 voxels: small components, spread addresses
#pragma unroll
                for (int i = 0; i < kFields; ++i) merge_global(table + (int64_t)row * kFields + i, i, f[i]);
            }
        }
    }
    cache_fence();
    for (int slot = 0; slot < kSlots; ++slot)
        if (key[slot] >= 0) flush_slot(table, val[slot], key[slot], lane);
}

// the two launches of either form: the table's initial values, then the sweep
template <typename Policy>
int launch_moments(const typename Policy::Elem* elems, const int32_t* comp, const int32_t* row_of_root, int64_t Z, int64_t Y, int64_t X, int64_t rows,
                   int64_t* table, double bytes_per_voxel, hipStream_t s) {
    const int64_t n = Z * Y * X, entries = rows * kFields;
    hipLaunchKernelGGL(table_init_kernel, dim3((unsigned)((entries + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, (long long*)table, entries,
                       (int)Z, (int)Y, (int)X);
    VS_LAUNCH_CHECK();
    const int64_t per_wg = (int64_t)kWaves * kSpanSteps * 256;
    ProfScope prof(PK_POOL_MISC, 0.0, bytes_per_voxel * (double)n, s);
    hipLaunchKernelGGL(moments_kernel<Policy>, dim3((unsigned)((n + per_wg - 1) / per_wg)), dim3(kThreads), 0, s, elems, comp, row_of_root, (int)Z, (int)Y,
                       (int)X, n, (int)rows, (long long*)table);
    VS_LAUNCH_CHECK();
    return VS_OK;
}

}  // namespace

extern "C" int vs_component_moments(const uint8_t* labels, const int32_t* comp, const int32_t* row_of_root, int64_t Z, int64_t Y, int64_t X,
                                    int64_t rows, int64_t* table, void* stream) {
    VS_REQUIRE(extents_fit(Z, Y, X, 0), "component_moments: extents %lld x %lld x %lld - every extent must be at least 1 and the volume below 2^31 "
               "voxels (component ids are int32 voxel indices)", (long long)Z, (long long)Y, (long long)X);
    const int64_t n = Z * Y * X;
    VS_REQUIRE(rows >= 0 && rows <= n, "component_moments: %lld rows - a volume of %lld voxels has between 0 and that many components",
               (long long)rows, (long long)n);
    if (rows == 0) return VS_OK;
    VS_REQUIRE(labels && comp && row_of_root && table, "component_moments: null argument");
    VS_REQUIRE(((uintptr_t)labels | (uintptr_t)comp | (uintptr_t)row_of_root) % 4 == 0 && (uintptr_t)table % 8 == 0,
               "component_moments: labels, comp and row_of_root must be 4-byte, the table 8-byte aligned");
    return launch_moments<ByValue>(labels, comp, row_of_root, Z, Y, X, rows, table, 5.0, (hipStream_t)stream);      // labels and their four neighbouring rows; ids and rows once per run
}

extern "C" int vs_object_moments(const int32_t* objects, const int32_t* row_of_root, int64_t Z, int64_t Y, int64_t X, int64_t rows, int64_t* table,
                                 void* stream) {
    VS_REQUIRE(extents_fit(Z, Y, X, 0), "object_moments: extents %lld x %lld x %lld - every extent must be at least 1 and the volume below 2^31 "
               "voxels (object ids are int32 voxel indices)", (long long)Z, (long long)Y, (long long)X);
    const int64_t n = Z * Y * X;
    VS_REQUIRE(rows >= 0 && rows <= n, "object_moments: %lld rows - a volume of %lld voxels has between 0 and that many objects", (long long)rows,
               (long long)n);
    if (rows == 0) return VS_OK;
    VS_REQUIRE(objects && row_of_root && table, "object_moments: null argument");
    VS_REQUIRE((uintptr_t)objects % 16 == 0 && (uintptr_t)row_of_root % 4 == 0 && (uintptr_t)table % 8 == 0,
               "object_moments: objects must be 16-byte, row_of_root 4-byte, the table 8-byte aligned");
    return launch_moments<ById>(objects, nullptr, row_of_root, Z, Y, X, rows, table, 20.0, (hipStream_t)stream);     // ids and their four neighbouring rows
}
