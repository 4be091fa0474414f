// The overlap table of two labellings (gfx950): from the roots a and b that vs_label_components gave two volumes of the same
// extents, the list of (root in a, root in b, voxels that have both) - what matching true and predicted objects starts from
// (include/volseg_hip.h has the contract; utilities/object_scores.py is the Python layer and the host route that gives the same
// integers).  The key of a voxel is (a << 32) | b; a voxel whose skip byte is set has none.  Integer adds commute: atomics are
// allowed and, sorted by key, the table is the same bits on every run.
//
// Both sweeps give a wave a contiguous span of kSpanSteps x 256 voxels.  Per step the loads of four groups of 64 consecutive
// voxels are issued together; lane l of a group holds voxel 64 k + l.  A voxel starts a run when it is not skipped and the voxel
// before it in its row is skipped or has another key (or there is none: x == 0); the voxel before a group's lane 0 comes from
// the group before it, at a step's first group from memory.
//
// vs_overlap_runs: one ballot and popcount per group, the wave's total to LDS, one 64-bit add per workgroup.
//
// vs_overlap_table: an open-addressing table (linear probing) in device memory.  What reaches it:
//  * A group with at most kRounds runs is taken key by key: the first voxel left names a key, one ballot finds every voxel of
//    the group that has it, and the popcount goes into the wave's cache - one (key, count) pair per LANE, in registers, two
//    ways: a hash of the key picks a lane and its neighbour.  A pair leaves for the table when another key takes its lane and
//    at the end of the span.
//    A solid volume therefore issues one insertion per wave (8192 voxels), a volume of a few big objects one per wave and
//    object, and the keys that every wave meets - background on background - are not hammered once per run.
//  * A group with more runs than that is debris: each run's first lane inserts the run's length itself, all of them at once, on
//    addresses the hash spreads.  (Lane 0 leads what is left of a run that began in the group before.)
//  An insertion is a bounded probe: read the slot; on the key, stop; on the free mark, compare-and-swap the key in (on losing
//  the race to the same key, stop as well); else the next slot - `slots` steps at most, then used[1] = 1 and the lane gives up.
//  The count is one 64-bit add - none where a claim brings one voxel: counts start at 1.  Claimed slots are counted per lane and summed once per wave into used[0].
#include <algorithm>

#include "common.h"
#include "prof.h"

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kSpanSteps = 32;                 // steps of 256 voxels a wave takes over its contiguous span
constexpr int kRounds = 16;                    // runs a group may have and still be taken key by key through the cache
constexpr unsigned long long kFree = ~0ull;    // no key: roots are below 2^31

// the four groups of a step: key halves, "has a key", and the run starts as one ballot per group
struct Step {
    int a[4], b[4];
    bool live[4];
    uint64_t starts[4], lives[4];
};

__device__ __forceinline__ void load_step(Step& s, const int* __restrict__ a, const int* __restrict__ b, const uint8_t* __restrict__ skip, int64_t sb,
                                          int64_t n, uint32_t X, int lane) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t p = sb + 64 * k + lane;
        const bool in = p < n;
        s.a[k] = in ? a[p] : -1;
        s.b[k] = in ? b[p] : -1;
        s.live[k] = in && !(skip && skip[p]);
    }
    // the voxel in front of the step, for lane 0 of the first group
    int fa = -1, fb = -1;
    bool flive = false;
    if (lane == 0 && sb > 0 && sb < n) {
        fa = a[sb - 1];
        fb = b[sb - 1];
        flive = !(skip && skip[sb - 1]);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t p = sb + 64 * k + lane;
        const uint32_t pu = p < n ? (uint32_t)p : 0u, x = pu % X;
        int pa = __shfl_up(s.a[k], 1, 64), pb = __shfl_up(s.b[k], 1, 64);
        int plive = __shfl_up((int)s.live[k], 1, 64);
        const int ea = k == 0 ? fa : __shfl(s.a[k > 0 ? k - 1 : 0], 63, 64), eb = k == 0 ? fb : __shfl(s.b[k > 0 ? k - 1 : 0], 63, 64);
        const int elive = k == 0 ? (int)flive : __shfl((int)s.live[k > 0 ? k - 1 : 0], 63, 64);
        if (lane == 0) { pa = ea; pb = eb; plive = elive; }
        const bool start = s.live[k] && (x == 0 || !plive || pa != s.a[k] || pb != s.b[k]);
        s.starts[k] = __ballot(start);
        s.lives[k] = __ballot(s.live[k]);
    }
}

__global__ __launch_bounds__(kThreads) void overlap_runs_kernel(const int* __restrict__ a, const int* __restrict__ b, const uint8_t* __restrict__ skip,
                                                              int64_t n, uint32_t X, unsigned long long* __restrict__ runs) {
    __shared__ long long wave_total[kWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t base = ((int64_t)blockIdx.x * kWaves + wave) * kSpanSteps * 256;
    long long total = 0;                                                // uniform over the wave
    for (int step = 0; step < kSpanSteps; ++step) {
        const int64_t sb = base + (int64_t)step * 256;
        if (sb >= n) break;                                             // uniform over the wave
        Step s;
        load_step(s, a, b, skip, sb, n, X, lane);
#pragma unroll
        for (int k = 0; k < 4; ++k) total += __popcll(s.starts[k]);
    }
    if (lane == 0) wave_total[wave] = total;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long sum = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) sum += wave_total[w];
        if (sum) atomicAdd(runs, (unsigned long long)sum);
    }
}

__device__ __forceinline__ unsigned long long mix(unsigned long long h) {
    h ^= h >> 33; h *= 0xff51afd7ed558ccdull;
    h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53ull;
    return h ^ (h >> 33);
}

// count voxels more for `key`; returns 1 when this lane claimed a free slot.  At most mask + 1 probes.  The slot is read before the
// compare-and-swap: a slot every wave meets is then read, not swapped at, and a compare-and-swap costs several reads.  Atomics
// are what debris pays for, so a claim brings its first voxel with it: every count starts at 1 and the claimer adds its run's
// length minus one - nothing at all for a run of one voxel, which is most of debris (DESIGN 3g has what was measured).
__device__ __forceinline__ int insert(unsigned long long* __restrict__ keys, unsigned long long* __restrict__ counts, unsigned long long mask,
                                      unsigned long long* __restrict__ used, unsigned long long key, long long count) {
    unsigned long long slot = mix(key) & mask;
    for (unsigned long long probe = 0; probe <= mask; ++probe, slot = (slot + 1) & mask) {
        unsigned long long seen = __hip_atomic_load(keys + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        int claimed = 0;
        if (seen == kFree) {
            seen = atomicCAS(keys + slot, kFree, key);                  // 64 bits, agent scope
            claimed = seen == kFree;
            if (claimed) seen = key;
        }
        if (seen == key) {
            count -= claimed;                                            // a slot's count starts at 1: the claim itself is one voxel
            if (count) atomicAdd(counts + slot, (unsigned long long)count);
            return claimed;
        }
    }
    __hip_atomic_store(used + 1, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // the table is full: give up, never spin
    return 0;
}

__global__ __launch_bounds__(kThreads) void fill_ones_kernel(unsigned long long* __restrict__ p, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) p[i] = 1ull;
}

__global__ __launch_bounds__(kThreads) void overlap_table_kernel(const int* __restrict__ a, const int* __restrict__ b, const uint8_t* __restrict__ skip,
                                                               int64_t n, uint32_t X, unsigned long long* __restrict__ keys,
                                                               unsigned long long* __restrict__ counts, unsigned long long mask,
                                                               unsigned long long* __restrict__ used) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t base = ((int64_t)blockIdx.x * kWaves + wave) * kSpanSteps * 256;
    unsigned long long cached_key = kFree;                              // this lane's pair of the wave's cache
    long long cached_count = 0;
    int claims = 0;
    for (int step = 0; step < kSpanSteps; ++step) {
        const int64_t sb = base + (int64_t)step * 256;
        if (sb >= n) break;                                             // uniform over the wave
        Step s;
        load_step(s, a, b, skip, sb, n, X, lane);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint64_t lives = s.lives[k];
            if (!lives) continue;                                       // uniform: 64 voxels without a key
            const uint64_t leaders = s.starts[k] | (lives & 1);         // lane 0 leads what is left of a run from the group before
            const unsigned long long key = ((unsigned long long)(uint32_t)s.a[k] << 32) | (uint32_t)s.b[k];
            if (__popcll(leaders) <= kRounds) {                         // uniform
                uint64_t rest = lives;
                while (rest) {                                          // at most kRounds turns: a key has a run of its own
                    const int first = __ffsll((unsigned long long)rest) - 1;
                    const int wa = __shfl(s.a[k], first, 64), wb = __shfl(s.b[k], first, 64);
                    const unsigned long long want = ((unsigned long long)(uint32_t)wa << 32) | (uint32_t)wb;
                    const uint64_t members = __ballot(s.live[k] && key == want);
                    // two ways: the key's home lane and its neighbour - the lane that holds the key, else a free one, else home
                    const int home = (int)((((uint32_t)wa * 0x9E3779B1u) ^ ((uint32_t)wb * 0x85EBCA6Bu)) >> 26);
                    const bool way = (lane | 1) == (home | 1);
                    const uint64_t holds = __ballot(way && cached_key == want), free_way = __ballot(way && cached_key == kFree);
                    const int target = holds ? __ffsll((unsigned long long)holds) - 1 : free_way ? __ffsll((unsigned long long)free_way) - 1 : home;
                    if (lane == target) {
                        if (cached_key != want) {
                            if (cached_key != kFree) claims += insert(keys, counts, mask, used, cached_key, cached_count);
                            cached_key = want;
                            cached_count = 0;
                        }
                        cached_count += __popcll(members);
                    }
                    rest &= ~members;
                }
            } else if ((leaders >> lane) & 1) {
                const uint64_t upper = leaders & ~(((uint64_t)2 << lane) - 1);                 // lane 63: 2 << 63 wraps to 0, minus 1 = every bit
                const int end = upper ? __ffsll((unsigned long long)upper) - 2 : 63;
                const uint64_t mine = (((uint64_t)2 << end) - 1) & ~(((uint64_t)1 << lane) - 1);
                claims += insert(keys, counts, mask, used, key, __popcll(lives & mine));      // skipped voxels only follow a run's end
            }
        }
    }
    if (cached_key != kFree) claims += insert(keys, counts, mask, used, cached_key, cached_count);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) claims += __shfl_xor(claims, o, 64);
    if (lane == 0 && claims) atomicAdd(used, (unsigned long long)claims);
}

int check_arguments(const char* what, const void* a, const void* b, int64_t n, int64_t X) {
    VS_REQUIRE(n > 0 && n < (1LL << 31) && X > 0 && n % X == 0, "%s: %lld voxels in rows of %lld - between 1 and 2^31 - 1 voxels in whole rows",
               what, (long long)n, (long long)X);
    VS_REQUIRE(a && b, "%s: null argument", what);
    VS_REQUIRE(((uintptr_t)a | (uintptr_t)b) % 4 == 0, "%s: a and b must be 4-byte aligned", what);
    return VS_OK;
}

constexpr int64_t kPerWorkgroup = (int64_t)kWaves * kSpanSteps * 256;

}  // namespace

extern "C" int vs_overlap_runs(const int32_t* a, const int32_t* b, const uint8_t* skip, int64_t n, int64_t X, int64_t* runs, void* stream) {
    if (int rc = check_arguments("overlap_runs", a, b, n, X)) return rc;
    VS_REQUIRE(runs && (uintptr_t)runs % 8 == 0, "overlap_runs: runs must be 8-byte aligned device memory");
    hipStream_t s = (hipStream_t)stream;
    VS_CHECK_HIP(hipMemsetAsync(runs, 0, sizeof(int64_t), s));
    ProfScope prof(PK_POOL_MISC, 0.0, (skip ? 9.0 : 8.0) * (double)n, s);
    hipLaunchKernelGGL(overlap_runs_kernel, dim3((unsigned)((n + kPerWorkgroup - 1) / kPerWorkgroup)), dim3(kThreads), 0, s, a, b, skip, n, (uint32_t)X,
                       (unsigned long long*)runs);
    VS_LAUNCH_CHECK();
    return VS_OK;
}

extern "C" int vs_overlap_table(const int32_t* a, const int32_t* b, const uint8_t* skip, int64_t n, int64_t X, uint64_t* keys, int64_t* counts,
                                int64_t slots, int64_t* used, void* stream) {
    if (int rc = check_arguments("overlap_table", a, b, n, X)) return rc;
    VS_REQUIRE(slots >= 1 && (slots & (slots - 1)) == 0, "overlap_table: %lld slots - the table size is a power of two", (long long)slots);
    VS_REQUIRE(keys && counts && used && ((uintptr_t)keys | (uintptr_t)counts | (uintptr_t)used) % 8 == 0,
               "overlap_table: keys, counts and used must be 8-byte aligned device memory");
    hipStream_t s = (hipStream_t)stream;
    VS_CHECK_HIP(hipMemsetAsync(keys, 0xFF, (size_t)slots * sizeof(uint64_t), s));
    hipLaunchKernelGGL(fill_ones_kernel, dim3((unsigned)std::min<int64_t>((slots + kThreads - 1) / kThreads, 16 * persistent_workgroups())), dim3(kThreads), 0,
                       s, (unsigned long long*)counts, slots);
    VS_LAUNCH_CHECK();
    VS_CHECK_HIP(hipMemsetAsync(used, 0, 2 * sizeof(int64_t), s));
    {
        ProfScope prof(PK_POOL_MISC, 0.0, (skip ? 9.0 : 8.0) * (double)n, s);
        hipLaunchKernelGGL(overlap_table_kernel, dim3((unsigned)((n + kPerWorkgroup - 1) / kPerWorkgroup)), dim3(kThreads), 0, s, a, b, skip, n,
                           (uint32_t)X, (unsigned long long*)keys, (unsigned long long*)counts, (unsigned long long)(slots - 1),
                           (unsigned long long*)used);
        VS_LAUNCH_CHECK();
    }
    int64_t host_used[2] = {0, 0};
    VS_CHECK_HIP(hipMemcpyAsync(host_used, used, sizeof(host_used), hipMemcpyDeviceToHost, s));
    VS_CHECK_HIP(hipStreamSynchronize(s));
    VS_REQUIRE(host_used[1] == 0, "overlap_table: the table of %lld slots is full - an insertion found no slot for its key; size it from vs_overlap_runs "
               "(a power of two at or above twice the runs)", (long long)slots);
    return VS_OK;
}
