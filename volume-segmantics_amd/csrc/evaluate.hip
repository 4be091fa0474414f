// Scoring a predicted label volume against ground truth (gfx950, HBM-bound byte work): the confusion matrix of two uint8
// volumes, for the whole volume or per slab (slab = H*W: one matrix per leading-axis slice).  Everything a segmentation score
// needs (per-class Dice, IoU, precision, recall, accuracy) follows from these integers on the host
// (utilities/evaluation.py).
//
// Shape of the kernel.  The volume is cut into items: at most kChunk consecutive voxels of ONE slab, so no item straddles a
// slab boundary.  A persistent grid takes contiguous runs of items; a workgroup keeps one 258-counter histogram per wave in
// LDS (256 pair codes t * K + p, then `ignored`, `invalid`), and when its next item belongs to another slab - or at its end -
// sums the four and issues one 64-bit global atomic per non-zero counter.  Integer sums: the result is the same bits
// whatever order workgroups arrive in.
//
// Label volumes are coherent: nearly every neighbour carries the same (truth, pred) pair, so one LDS atomic per voxel would
// have all 64 lanes of a wave serialise on one counter.  Two levels of aggregation come before any atomic:
//  * a lane whose 16 truth bytes and 16 prediction bytes are each one repeated value classifies ONE voxel, and the wave then
//    groups such lanes by code with ballots: one add of 16 * popcount per distinct code (a constant volume: one add of 1024
//    per wave step);
//  * any other lane walks its 16 voxels and adds once per run of equal codes.
// Random labels take the second path throughout; their adds spread over the counters and the LDS banks by themselves.
#include "common.h"

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kCodes = 258;                    // 256 pair codes, [256] ignored, [257] invalid
constexpr int kIgnored = 256, kInvalid = 257;
constexpr int64_t kChunk = 1 << 16;            // voxels per item: 16 x 16-byte vectors per lane
constexpr int kUnroll = 4;                     // 16-byte load pairs in flight per lane

// truth byte -> class through the workgroup's LDS copy of the table (255 ignore, 254 invalid, else < K), then the counter index.
// Every returned index is < kCodes, and < K * K unless it is one of the two dropped counters, whatever the two bytes are.
__device__ __forceinline__ int classify(const uint8_t* lut, uint32_t tb, uint32_t pb, int K) {
    const int tc = lut[tb & 0xff];
    pb &= 0xff;
    return tc == 255 ? kIgnored : (tc == 254 || pb >= (uint32_t)K) ? kInvalid : tc * K + (int)pb;
}

__device__ __forceinline__ bool one_byte_repeated(const uint4 v) {
    return v.x == v.y && v.y == v.z && v.z == v.w && v.x == (v.x & 0xff) * 0x01010101u;
}

// one 16-voxel vector per active lane into the wave's histogram; every lane of the wave must call this (ballots inside)
__device__ __forceinline__ void count_vector(uint32_t* hist, const uint8_t* lut, bool active, const uint4 t, const uint4 p, int K) {
    const bool flat = active && one_byte_repeated(t) && one_byte_repeated(p);
    const int code = classify(lut, t.x, p.x, K);
    uint64_t rest = __ballot(flat);
    const int lane = threadIdx.x & 63;
    while (rest) {                               // wave-uniform: one turn per distinct code among the flat lanes
        const int leader = __ffsll((unsigned long long)rest) - 1;
        const int c = __shfl(code, leader, 64);
        const uint64_t same = __ballot(flat && code == c);
        if (lane == leader) atomicAdd(hist + c, 16u * (uint32_t)__popcll(same));
        rest &= ~same;
    }
    if (active && !flat) {
        const uint32_t tw[4] = {t.x, t.y, t.z, t.w}, pw[4] = {p.x, p.y, p.z, p.w};
        int cur = code;
        uint32_t run = 0;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int c = classify(lut, tw[j >> 2] >> (8 * (j & 3)), pw[j >> 2] >> (8 * (j & 3)), K);
            if (c != cur) {
                atomicAdd(hist + cur, run);      // run >= 1 here: j = 0 has c == cur
                cur = c;
                run = 0;
            }
            ++run;
        }
        atomicAdd(hist + cur, run);
    }
}

__global__ __launch_bounds__(kThreads) void confusion_kernel(const uint8_t* __restrict__ truth, const uint8_t* __restrict__ pred,
                                                           int64_t n, int K, const uint8_t* __restrict__ truth_lut,
                                                           int64_t slab_len, int64_t chunks_per_slab, int64_t items,
                                                           int64_t items_per_wg, unsigned long long* __restrict__ counts,
                                                           unsigned long long* __restrict__ dropped) {
    __shared__ uint32_t hist[kWaves][kCodes + 2];
    __shared__ uint8_t lut[256];
    const int tid = threadIdx.x, wave = tid >> 6;
    {   // the table with the class range folded in: nothing >= K other than the two marks leaves it
        const int v = truth_lut ? truth_lut[tid] : tid;
        lut[tid] = (uint8_t)(truth_lut && v == 255 ? 255 : v >= K ? 254 : v);
    }
    for (int i = tid; i < kWaves * (kCodes + 2); i += kThreads) (&hist[0][0])[i] = 0;
    __syncthreads();

    const int64_t first = (int64_t)blockIdx.x * items_per_wg;
    const int64_t last = first + items_per_wg < items ? first + items_per_wg : items;
    int64_t cur_slab = -1;
    for (int64_t item = first; item < last; ++item) {
        const int64_t slab = item / chunks_per_slab, chunk = item - slab * chunks_per_slab;
        if (slab != cur_slab) {
            if (cur_slab >= 0) {                 // flush: the four wave histograms -> one global add per non-zero counter
                __syncthreads();
                for (int i = tid; i < kCodes; i += kThreads) {
                    unsigned long long s = 0;
#pragma unroll
                    for (int w = 0; w < kWaves; ++w) { s += hist[w][i]; hist[w][i] = 0; }
                    if (s) {
                        if (i >= kIgnored) atomicAdd(dropped + cur_slab * 2 + (i - kIgnored), s);
                        else if (i < K * K) atomicAdd(counts + cur_slab * K * K + i, s);
                    }
                }
                __syncthreads();
            }
            cur_slab = slab;
        }
        const int64_t slab_end = (slab + 1) * slab_len < n ? (slab + 1) * slab_len : n;
        const int64_t a = slab * slab_len + chunk * kChunk;
        const int64_t b = a + kChunk < slab_end ? a + kChunk : slab_end;
        if (a >= b) continue;
        // [a, b) = up to 15 head voxels, whole 16-byte vectors [va, vb), up to 15 tail voxels (the bases are 16-byte aligned)
        int64_t va = (a + 15) & ~(int64_t)15, vb = b & ~(int64_t)15;
        if (va > vb) va = vb = b;                // no 16-byte boundary inside [a, b]: fewer than 16 voxels, all of them "head"
        if (tid < 32) {
            const int64_t i = tid < 16 ? a + tid : vb + (tid - 16);
            const int64_t end = tid < 16 ? va : b;
            if (i < end) atomicAdd(&hist[wave][classify(lut, truth[i], pred[i], K)], 1u);
        }
        const uint4* tv = reinterpret_cast<const uint4*>(truth + va);
        const uint4* pv = reinterpret_cast<const uint4*>(pred + va);
        const int64_t nv = (vb - va) >> 4;
        for (int64_t v0 = 0; v0 < nv; v0 += kThreads * kUnroll) {     // bounds are uniform over the workgroup
            uint4 t[kUnroll], p[kUnroll];
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                const int64_t v = v0 + u * kThreads + tid;
                t[u] = p[u] = make_uint4(0u, 0u, 0u, 0u);
                if (v < nv) { t[u] = tv[v]; p[u] = pv[v]; }
            }
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) count_vector(hist[wave], lut, v0 + u * kThreads + tid < nv, t[u], p[u], K);
        }
    }
    if (cur_slab >= 0) {
        __syncthreads();
        for (int i = tid; i < kCodes; i += kThreads) {
            unsigned long long s = 0;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) s += hist[w][i];
            if (s) {
                if (i >= kIgnored) atomicAdd(dropped + cur_slab * 2 + (i - kIgnored), s);
                else if (i < K * K) atomicAdd(counts + cur_slab * K * K + i, s);
            }
        }
    }
}

}  // namespace

extern "C" int vs_confusion_matrix(const uint8_t* truth, const uint8_t* pred, int64_t n, int classes, const uint8_t* truth_lut,
                                   int64_t slab_len, int64_t* counts, int64_t* dropped, void* stream) {
    VS_REQUIRE(truth && pred && counts && dropped && n >= 1 && slab_len >= 1, "confusion_matrix: bad arguments");
    VS_REQUIRE(classes >= 1 && classes <= 16,
               "confusion_matrix: %d classes - the kernel serves 1..16 (the pair code t * K + p is one byte)", classes);
    VS_REQUIRE(((uintptr_t)truth | (uintptr_t)pred) % 16 == 0, "confusion_matrix: volumes must be 16-byte aligned");
    if (slab_len > n) slab_len = n;
    const int64_t nslabs = (n + slab_len - 1) / slab_len;
    const int64_t chunks_per_slab = (slab_len + kChunk - 1) / kChunk;
    VS_REQUIRE(nslabs < (1LL << 40) / chunks_per_slab, "confusion_matrix: too many slabs");
    const int64_t items = nslabs * chunks_per_slab;
    hipStream_t s = (hipStream_t)stream;
    VS_CHECK_HIP(hipMemsetAsync(counts, 0, (size_t)nslabs * classes * classes * sizeof(int64_t), s));
    VS_CHECK_HIP(hipMemsetAsync(dropped, 0, (size_t)nslabs * 2 * sizeof(int64_t), s));
    // The LDS counters are 32-bit, and between two flushes a workgroup sees at most items_per_wg items of kChunk = 2^16 voxels:
    // items_per_wg <= 2^15 keeps that at or below 2^31 < 2^32.  Sums across workgroups are 64-bit.
    int64_t grid = persistent_workgroups();
    if (grid > items) grid = items;
    int64_t items_per_wg = (items + grid - 1) / grid;
    if (items_per_wg > (1 << 15)) items_per_wg = 1 << 15;
    grid = (items + items_per_wg - 1) / items_per_wg;
    VS_REQUIRE(grid < (1LL << 31), "confusion_matrix: volume too large");
    hipLaunchKernelGGL(confusion_kernel, dim3((unsigned)grid), dim3(kThreads), 0, s, truth, pred, n, classes, truth_lut, slab_len,
                       chunks_per_slab, items, items_per_wg, (unsigned long long*)counts, (unsigned long long*)dropped);
    VS_LAUNCH_CHECK();
    return VS_OK;
}
