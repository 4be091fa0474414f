// The strip-walk convolution kernels: the HBM-bound full-resolution end of the network (<= 16 couts, Cin within one chunk,
// large images) - the last decoder layers, the segmentation head in training and in prediction, the head's data gradient
// and the fused last decoder block of the evaluation forward.
//
// The full-resolution decoder layers (-> 16 channels at H x W), the segmentation head and the head's data gradient have so
// little matrix work per pixel that the LDS-staged tile kernel (conv_igemm.hip) spends its time in barriers and load
// latency.  Here every wave is on its own: it owns a 16-pixel-wide column strip of RH output rows and walks down it with a
// rolling window of input rows held as MFMA B fragments that are loaded STRAIGHT from global memory (one 16-byte buffer
// load per lane: pixel = column + kw - 1, channels 8*(lane>>4)..; padding = out-of-range offset = zeros).  Each new output
// row costs 3 loads (the next input row at the three kw shifts; the 3x reuse across kh lives in registers, the rest in
// L1), 9 MFMAs against the weight slab (staged once per workgroup in LDS) and its stores.  No barriers in the loop, many
// independent waves per SIMD.
//
//   conv_direct_kernel        one 3x3 layer -> <= 16 couts: NHWC store with affine / activation / BatchNorm statistics, or
//                             the 2x2 sum-pooled store of a data gradient through nearest-x2 upsampling
//   conv_head_kernel          <= 4 classes, four output rows per accumulator tile: fp32 NCHW logits, or labels /
//                             probabilities / packed keys written into the output volume itself
//   conv_direct_pair_kernel   two chained layers in one launch, the tensor between them never stored
//   head_dgrad_planes_kernel  the head's data gradient gathered from the loss gradient's fp32 planes
//
// Every piece the kernels share is written once, in front of them: the wave -> strip decode, the weight slab staging (stage_slabs), the
// row loader, the per-lane affine, the activation, the 4-value store and the three rolling accumulators of a 3x3 walk; on
// the host, strip_geom.  conv_plan (conv_igemm.hip) decides which launches come here.
#pragma once
#include <hip/hip_fp16.h>

#include <algorithm>

#include "conv_common.h"
#include "prof.h"

namespace strip {

constexpr int kPS = 64;  // LDS bytes per staged pixel / weight row: unpadded; the 16-byte segment s of a patch pixel in patch
                         // column pw lives in slot s ^ ((pw >> 1) & 3), of weight row r in slot s ^ ((r >> 1) & 3).  With
                         // gfx950's ds_read_b128 lane groups this XOR makes the fragment reads conflict-free (tools/lds_bank_sim.py;
                         // 80-byte padded rows are 2-way conflicted, 96-byte ones conflict-free but 50 % bigger).  Keying the
                         // patch swizzle on the column keeps the kh tap offsets plain constants.
__device__ __forceinline__ int swz(int row, int key, int seg) { return row * kPS + ((seg ^ ((key >> 1) & 3)) << 4); }

constexpr int kOob = (int)0x80000000;           // lane offset of a buffer store that must not land
constexpr int kSlabBytes = 9 * 16 * kPS;        // a 3x3 weight slab of 16 couts: row = tap * 16 + cout

struct DirectGeom {
    int strips_w, chunks_h, RH;      // column strips per row, row chunks per image, rows per chunk
    unsigned sw_magic, ch_magic;     // x / strips_w, x / chunks_h by umulhi
    int nwaves;
};

// ---- the shared pieces ------------------------------------------------------------------------------------------------------
// wave gw -> (image n, row chunk hc, column strip ws): strips of one row chunk are neighbours, chunks of one image follow
struct Strip { int n, hc, ws; };
__device__ __forceinline__ Strip strip_of(int gw, const DirectGeom& g) {
    const int q = g.strips_w == 1 ? gw : (int)__umulhi((unsigned)gw, g.sw_magic);
    const int n = g.chunks_h == 1 ? q : (int)__umulhi((unsigned)q, g.ch_magic);
    return Strip{n, q - n * g.chunks_h, gw - q * g.strips_w};
}

// w [Cout][9][Cin] -> the swizzled slab wl (kSlabBytes + a 64-byte dump slot for the items past it), by all 256 threads of
// the workgroup; couts past Cout and the channel tail are zeros.  Visible behind the caller's barrier.  NS slabs are staged
// together: the loads of a round are all issued before the first LDS write waits for one of them.
template <typename T, int NS>
__device__ __forceinline__ void stage_slabs(char* const (&wl)[NS], const void* const (&w)[NS], const int (&Cout)[NS], const int (&Cin)[NS]) {
    constexpr int EPS = CT<T>::EPS, WTOTAL = 9 * 16 * 4, WITEMS = (WTOTAL + 255) / 256;
    __amdgpu_buffer_rsrc_t rw[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) rw[s] = make_rsrc(w[s], Cout[s] * 9 * Cin[s] * (int)sizeof(T));
#pragma unroll
    for (int i = 0; i < WITEMS; ++i) {
        const int item = threadIdx.x + i * 256;
        const int row = item >> 2, seg = item & 3;
        const int tap = row / 16, nr = row % 16;
        uint4 v[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const bool ok = item < WTOTAL && nr < Cout[s] && seg * EPS < Cin[s];
            v[s] = bload(rw[s], ok ? ((nr * 9 + tap) * Cin[s] + seg * EPS) * (int)sizeof(T) : -1, 0);
        }
        const int dst = item < WTOTAL ? swz(row, row, seg) : kSlabBytes;
#pragma unroll
        for (int s = 0; s < NS; ++s) *reinterpret_cast<uint4*>(wl[s] + dst) = v[s];
    }
}

// Input rows of image n as MFMA B fragments: lane (lq, lr) reads channels lq * EPS.. of column w0 + lr + kw - 1 for the three
// kw shifts (byte offsets inside an input row; -1 = zero: padding column / channel tail).  up0 = 1: the source is at half
// resolution (nearest x2 upsampling).
struct RowLoader {
    __amdgpu_buffer_rsrc_t rx;
    int coff[3], rowbytes, Hin, up0;
};
template <typename T>
__device__ __forceinline__ RowLoader row_loader(const ConvParams& p, int n, int w0, int up0, int lq, int lr) {
    constexpr int EPS = CT<T>::EPS;
    RowLoader L;
    const int H0 = p.Hin >> up0, W0 = p.Win >> up0;
    L.rowbytes = W0 * p.C0 * (int)sizeof(T);
    L.Hin = p.Hin;
    L.up0 = up0;
    L.rx = make_rsrc((const T*)p.src0 + (size_t)n * H0 * W0 * p.C0, H0 * L.rowbytes);
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
        const int col = w0 + lr + kw - 1;
        L.coff[kw] = (col >= 0 && col < p.Win && lq * EPS < p.C0) ? ((col >> up0) * p.C0 + lq * EPS) * (int)sizeof(T) : -1;
    }
    return L;
}
__device__ __forceinline__ void load_row(const RowLoader& L, int hi, uint4 (&x)[3]) {          // input row hi at the three kw shifts
    const bool ok = hi >= 0 && hi < L.Hin;
    const int soff = ok ? (hi >> L.up0) * L.rowbytes : 0;
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) x[kw] = bload(L.rx, ok ? L.coff[kw] : -1, soff);
}

// scale / shift of channels c .. c + 3 (1 / 0 where the pointer is null or the channel is past Cout)
__device__ __forceinline__ void load_affine4(const float* scale, const float* shift, int c, int Cout, float4& sc, float4& sh) {
    float a[4] = {1.f, 1.f, 1.f, 1.f}, b[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 4; ++r)
        if (c + r < Cout) { if (scale) a[r] = scale[c + r]; if (shift) b[r] = shift[c + r]; }
    sc = make_float4(a[0], a[1], a[2], a[3]); sh = make_float4(b[0], b[1], b[2], b[3]);
}
__device__ __forceinline__ void affine4(float (&v)[4], const float4& sc, const float4& sh) {
    v[0] = v[0] * sc.x + sh.x; v[1] = v[1] * sc.y + sh.y; v[2] = v[2] * sc.z + sh.z; v[3] = v[3] * sc.w + sh.w;
}
// relu: 0 = none, 1 = ReLU, 2 = swish
__device__ __forceinline__ void activate4(float (&v)[4], int relu) {
    if (relu == 1) { v[0] = fmaxf(v[0], 0.f); v[1] = fmaxf(v[1], 0.f); v[2] = fmaxf(v[2], 0.f); v[3] = fmaxf(v[3], 0.f); }
    else if (relu == 2) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = v[r] / (1.f + __expf(-v[r]));
    }
}

// four consecutive channels in T's storage format as ONE buffer store (b64 / b128); lane_off = kOob: nothing is written
template <typename T>
__device__ __forceinline__ void store4(__amdgpu_buffer_rsrc_t ro, int lane_off, int row_off, const float (&v)[4]) {
    if constexpr (sizeof(T) == 2) {
        uint2 pk;
        pk.x = pack2<T>(v[0], v[1]);
        pk.y = pack2<T>(v[2], v[3]);
        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(__attribute__((ext_vector_type(2))) unsigned int, pk), ro, lane_off, row_off, 0);
    } else {
        __builtin_amdgcn_raw_buffer_store_b128(u32x4{__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3])}, ro, lane_off, row_off, 0);
    }
}

// Input-row major 3x3 walk: input row hi feeds output rows hi+1 (kh = 0), hi (kh = 1) and hi-1 (kh = 2), whose accumulators
// a2, a1, a0 roll down by one slot per row.  x(kw): row hi at column shift kw, fetched beside that shift's weight fragments
// (registers of the input ring, or the pair kernel's LDS row); wl: the layer's slab; wb: swz(lr, lr, lq).
// PIN keeps the nine weight fragments in LDS, re-read every row, and not in 36 registers hoisted out of the row loop.
template <typename T, bool PIN, typename X>
__device__ __forceinline__ void row_into3(f32x4& a0, f32x4& a1, f32x4& a2, const char* wl, int wb, X x) {
    if (PIN) asm volatile("" : "+v"(wb));
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
        const uint4 xf = x(kw);
        const uint4 w0f = *reinterpret_cast<const uint4*>(wl + ((0 * 3 + kw) * 16) * kPS + wb);
        const uint4 w1f = *reinterpret_cast<const uint4*>(wl + ((1 * 3 + kw) * 16) * kPS + wb);
        const uint4 w2f = *reinterpret_cast<const uint4*>(wl + ((2 * 3 + kw) * 16) * kPS + wb);
        mma16<T>(a2, w0f, xf);
        mma16<T>(a1, w1f, xf);
        mma16<T>(a0, w2f, xf);
    }
}
// a0 has been read: the next output row moves into it
__device__ __forceinline__ void roll3(f32x4& a0, f32x4& a1, f32x4& a2) { a0 = a1; a1 = a2; a2 = f32x4{0.f, 0.f, 0.f, 0.f}; }

// ---- one shallow layer ------------------------------------------------------------------------------------------------------
// MODE 0: NHWC store in T (optional per-channel affine + ReLU, optional statistics); 1: 2x2 sum-pooled NHWC store (dgrad
// through nearest-x2 upsampling).  (The segmentation head has its own kernel below.)
// Every row iteration issues the same number of loads and (offset-masked, never skipped) buffer stores, so the waits on
// the input ring are counted ones and kD rows stay in flight per wave.
template <typename T, int MODE>
__global__ __launch_bounds__(256, 4) void conv_direct_kernel(ConvParams p, DirectGeom g) {
    constexpr int kD = MODE == 0 ? 2 : 4;   // input rows in flight
    __shared__ __attribute__((aligned(16))) char wl[kSlabBytes + 64];
    asm volatile("" ::"s"(p.src0), "s"(p.w), "s"(p.out), "s"(p.C0), "s"(p.up0), "s"(p.Hin), "s"(p.Win), "s"(p.Hout), "s"(p.Wout),
                 "s"(p.Cout), "s"(p.scale), "s"(p.shift), "s"(p.relu), "s"(p.stats_partial), "s"(g.strips_w), "s"(g.chunks_h),
                 "s"(g.RH), "s"(g.sw_magic), "s"(g.ch_magic), "s"(g.nwaves));   // one batch of kernel-argument loads
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lq = lane >> 4, lr = lane & 15;
    stage_slabs<T, 1>({wl}, {p.w}, {p.Cout}, {p.C0});   // once per workgroup
    __syncthreads();
    const int gw = blockIdx.x * 4 + wave;                   // this wave's strip
    if (gw >= g.nwaves) return;
    const Strip st = strip_of(gw, g);
    const int n = st.n, w0 = st.ws * 16, h0 = st.hc * g.RH, h1 = min(p.Hout, h0 + g.RH);
    const RowLoader rows = row_loader<T>(p, n, w0, p.up0, lq, lr);
    const int wbase_l = swz(lr, lr, lq);

    // output addressing: one descriptor per image, per-lane byte offset of (row 0, this lane's column, its first cout)
    const int wo = w0 + lr;
    const bool inw = wo < p.Wout;
    __amdgpu_buffer_rsrc_t ro;
    int ooff, orow;                                          // lane offset inside an output row; bytes per output row
    if constexpr (MODE == 0) {
        ro = make_rsrc((T*)p.out + (size_t)n * p.Hout * p.Wout * p.Cout, p.Hout * p.Wout * p.Cout * (int)sizeof(T));
        orow = p.Wout * p.Cout * (int)sizeof(T);
        ooff = (inw && lq * 4 < p.Cout) ? (wo * p.Cout + lq * 4) * (int)sizeof(T) : kOob;
    } else {
        const int Ho = p.Hout >> 1, Wo = p.Wout >> 1;
        ro = make_rsrc((T*)p.out + (size_t)n * Ho * Wo * p.Cout, Ho * Wo * p.Cout * (int)sizeof(T));
        orow = Wo * p.Cout * (int)sizeof(T);
        ooff = (inw && !(lr & 1) && lq * 4 < p.Cout) ? ((wo >> 1) * p.Cout + lq * 4) * (int)sizeof(T) : kOob;
    }
    float4 sc = make_float4(1.f, 1.f, 1.f, 1.f), sh = make_float4(0.f, 0.f, 0.f, 0.f);
    if (MODE != 1) load_affine4(p.scale, p.shift, lq * 4, p.Cout, sc, sh);
    const bool affine = MODE != 1 && (p.scale || p.shift);
    float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
    f32x4 prev = f32x4{0.f, 0.f, 0.f, 0.f};

    // a ring of kD input rows is in flight
    f32x4 a0 = f32x4{0.f, 0.f, 0.f, 0.f}, a1 = a0, a2 = a0;
    uint4 ring[kD][3];
#pragma unroll
    for (int u = 0; u < kD; ++u) load_row(rows, h0 - 1 + u, ring[u]);
    for (int base = h0 - 1; base <= h1; base += kD) {
#pragma unroll
        for (int u = 0; u < kD; ++u) {
            const int hi = base + u;
            if (hi > h1) break;
            row_into3<T, MODE != 0>(a0, a1, a2, wl, wbase_l, [&](int kw) { return ring[u][kw]; });   // (MODE 0: the 36 registers of the hoisted fragments are there)
            load_row(rows, hi + kD, ring[u]);
            const int h = hi - 1;                              // this output row is complete now
            const bool live = h >= h0;                         // (h < h1 always: hi <= h1)
            if (MODE == 0 && (p.stats_partial || p.stats_bins) && live && inw) {
#pragma unroll
                for (int r = 0; r < 4; ++r) { s1[r] += a0[r]; s2[r] += a0[r] * a0[r]; }
            }
            float v[4] = {a0[0], a0[1], a0[2], a0[3]};
            if constexpr (MODE == 1) {
#pragma unroll
                for (int r = 0; r < 4; ++r) { v[r] += prev[r]; v[r] += __shfl_xor(v[r], 1, 64); }
                prev = a0;
                store4<T>(ro, (live && (h & 1)) ? ooff : kOob, (h >> 1) * orow, v);
            } else {
                if (affine) affine4(v, sc, sh);
                activate4(v, p.relu);
                store4<T>(ro, live ? ooff : kOob, h * orow, v);
            }
            roll3(a0, a1, a2);
        }
    }
    if (MODE == 0 && (p.stats_partial || p.stats_bins)) {   // one partial row per wave: sum / sum of squares over the strip's pixels (or fixed-point bins)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) { s1[r] += __shfl_xor(s1[r], o, 64); s2[r] += __shfl_xor(s2[r], o, 64); }
            const int c = lq * 4 + r;
            if (lr == 0 && c < p.Cout) {
                if (p.stats_bins) {
                    unsigned long long* b = p.stats_bins + (size_t)(gw & (p.stats_nb - 1)) * 2 * p.Cout + c;
                    atomicAdd(b, (unsigned long long)__double2ll_rn((double)s1[r] * kStatScale1));
                    atomicAdd(b + p.Cout, (unsigned long long)__double2ll_rn((double)s2[r] * kStatScale2));
                } else {
                    p.stats_partial[((size_t)gw * 2 + 0) * p.Cout + c] = s1[r];
                    p.stats_partial[((size_t)gw * 2 + 1) * p.Cout + c] = s2[r];
                }
            }
        }
    }
}

// ---- the segmentation head's data gradient, straight from the loss gradient's planes ------------------------------------------
// da[y][x][ci] = sum over (window row r, column s, class k) of W[k][r][s][ci] * dl[k][y + 1 - r][x + 1 - s] with dl = dLoss / dlogits as
// autograd hands it over: fp32 NCHW planes of a FEW classes.  The strip kernel above wants it as a 16-channel NHWC tensor - a
// conversion launch (67 MB written, 14 of its 16 channels zero at two classes) on the critical path between the forward and the
// backward pass, then nine K = 32 MFMAs per 16 pixels that multiply mostly zeros.  Here the (tap, class) pairs ARE the K index:
// kk = 9 * k' .. with tap = kk / classes, class = kk % classes, 9 * classes <= 64 -> one or two MFMAs per 16 pixels, the B fragment
// gathered by each lane from the planes (8 scalar loads, L1 / L2 hits: every element is wanted by nine pixels), rounded to the
// storage type exactly as the conversion would have rounded it.  A wave owns a 16-column strip of RH rows, no LDS, no barriers.
// (Reference: the head's share of loss.backward(), vol_seg_2d_trainer.py:429.)
template <typename T, int NK>
__global__ __launch_bounds__(256, 4) void head_dgrad_planes_kernel(const float* __restrict__ dl, const T* __restrict__ w, T* __restrict__ out, int N, int classes,
                                                                  int H, int W, int C, DirectGeom g) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lq = lane >> 4, lr = lane & 15;
    const int gw = blockIdx.x * 4 + wave;
    if (gw >= g.nwaves) return;
    const Strip st = strip_of(gw, g);
    const int n = st.n, x = st.ws * 16 + lr, h0 = st.hc * g.RH, h1 = min(H, h0 + g.RH);
    const int KK = 9 * classes;
    // A fragments: A[m = ci = lr][kk = 32 qq + 8 lq + j] = W[class][tap][ci] (w: [classes][9][C], the forward's copy)
    uint4 af[NK];
    int poff[NK][8];          // per K slot: offset of its plane element relative to (class plane 0, row y, column x); kOob = no such slot / column outside
    int prow[NK][8];          // its window row r (the row bound check varies with y)
#pragma unroll
    for (int qq = 0; qq < NK; ++qq) {
        unsigned short a8[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int kk = 32 * qq + 8 * lq + j;
            const bool live = kk < KK;
            const int t = live ? kk / classes : 0, k = live ? kk - t * classes : 0;
            const int r = t / 3, sft = t - 3 * r;
            a8[j] = (live && lr < C) ? __builtin_bit_cast(unsigned short, w[((size_t)k * 9 + t) * C + lr]) : (unsigned short)0;
            const int xx = x + 1 - sft;
            poff[qq][j] = (live && xx >= 0 && xx < W) ? k * H * W + (1 - r) * W + xx : kOob;
            prow[qq][j] = r;
        }
        af[qq] = make_uint4((unsigned)a8[0] | ((unsigned)a8[1] << 16), (unsigned)a8[2] | ((unsigned)a8[3] << 16),
                            (unsigned)a8[4] | ((unsigned)a8[5] << 16), (unsigned)a8[6] | ((unsigned)a8[7] << 16));
    }
    const float* dn = dl + (size_t)n * classes * H * W;
    const __amdgpu_buffer_rsrc_t ro = make_rsrc(out + (size_t)n * H * W * C, H * W * C * (int)sizeof(T));
    const int ooff = (x < W && lq * 4 < C) ? (x * C + lq * 4) * (int)sizeof(T) : kOob;
    auto gather = [&](int y, float (&v)[NK][8]) {
        bool rok[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) { const int yy = y + 1 - r; rok[r] = yy >= 0 && yy < H && y < h1; }
#pragma unroll
        for (int qq = 0; qq < NK; ++qq)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const bool ok = poff[qq][j] != kOob && rok[prow[qq][j]];
                v[qq][j] = ok ? dn[(size_t)y * W + poff[qq][j]] : 0.f;
            }
    };
    float cur[NK][8], nxt[NK][8];
    gather(h0, cur);
    for (int y = h0; y < h1; ++y) {
        gather(y + 1, nxt);                                  // in flight while this row's MFMAs and store run
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int qq = 0; qq < NK; ++qq) {
            uint4 b;
            b.x = pack2<T>(cur[qq][0], cur[qq][1]); b.y = pack2<T>(cur[qq][2], cur[qq][3]);
            b.z = pack2<T>(cur[qq][4], cur[qq][5]); b.w = pack2<T>(cur[qq][6], cur[qq][7]);
            mma16<T>(acc, af[qq], b);
        }
        const float v[4] = {acc[0], acc[1], acc[2], acc[3]};
        store4<T>(ro, ooff, y * W * C * (int)sizeof(T), v);
#pragma unroll
        for (int qq = 0; qq < NK; ++qq)
#pragma unroll
            for (int j = 0; j < 8; ++j) cur[qq][j] = nxt[qq][j];
    }
}

// ---- two chained shallow layers in ONE launch (evaluation mode) ---------------------------------------------------------------
// smp's last decoder block at full resolution - Conv2dReLU(up(x), 32 -> 16) then Conv2dReLU(16 -> 16), BatchNorm folded into
// scale / shift (decoders/unet/decoder.py: DecoderBlock.conv1 / conv2, run by model(batch) at vol_seg_2d_predictor.py:44) - moves
// 1.6 + 2.1 GB per 128 x 512^2 batch as two strip-kernel launches, all but 0.5 + 1.1 GB of it the 16-channel tensor between them.
// Here a wave rolls BOTH layers down its strip: every row of the first layer's output goes - affine, ReLU, rounded to the storage
// type exactly as the first launch would have stored it - into a 16-pixel LDS row of the wave's own, from which the second layer
// reads its three column shifts as MFMA B fragments; the intermediate tensor never exists.  Strips are 14 output columns wide: lane
// lr of the 16-lane rows holds column w0 - 1 + lr of the FIRST layer (the one-pixel halo the second layer's 3 x 3 window needs), the
// second layer's lanes 0 and 15 compute nothing that is stored.  Rows / columns of the first layer's output outside the image are
// written as zeros - they are the second layer's zero padding.  Per output value the products and their order (kh-major taps,
// K = 32 MFMA k-steps over the same channel -> k mapping) are those of conv_direct_kernel / conv_igemm_kernel: bit-identical results
// (tests/test_hip_ops.py::test_direct_pair_equals_two_launches_bit_for_bit).  16-bit storage types only.  Measured: 1 034 us against 2 x 562 us
// per 128 x 512^2 batch, 0.8 % of a 512^3 prediction - the strip walk is bound by its MFMA + LDS-fragment issue (18 MFMAs and 22 LDS
// operations per 16-pixel row and wave), not by the 2.1 GB of HBM traffic the fusion removes.
template <typename T>
__global__ __launch_bounds__(256, 4) void conv_direct_pair_kernel(ConvParams p, ConvParams q, DirectGeom g) {
    constexpr int kD = 4;
    constexpr int kRowB = 18 * 32;                                   // one first-layer row of a wave: 16 pixels + a zero pixel each side, 16 channels
    __shared__ __attribute__((aligned(16))) char wl1[kSlabBytes + 64];
    __shared__ __attribute__((aligned(16))) char wl2[kSlabBytes + 64];
    __shared__ __attribute__((aligned(16))) char ybuf[4 * kRowB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lq = lane >> 4, lr = lane & 15;
    const int Cmid = p.Cout;
    char* yb = ybuf + wave * kRowB;
    stage_slabs<T, 2>({wl1, wl2}, {p.w, q.w}, {p.Cout, q.Cout}, {p.C0, Cmid});   // both weight slabs: once per workgroup
    // the halo pixels of this wave's row stay zero for good
    if (lane < 4) *reinterpret_cast<uint4*>(yb + (lane & 1) * 16 + (lane >> 1) * 17 * 32) = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();
    const int gw = blockIdx.x * 4 + wave;                            // this wave's strip
    if (gw >= g.nwaves) return;
    const Strip st = strip_of(gw, g);
    const int n = st.n, w0 = st.ws * 14 - 1, h0 = st.hc * g.RH, h1 = min(q.Hout, h0 + g.RH);      // lane lr: column w0 + lr of BOTH layers' outputs
    const RowLoader rows = row_loader<T>(p, n, w0, p.up0, lq, lr);
    const int wbase_l = swz(lr, lr, lq);
    // the second layer's output: one descriptor per image, lane offset inside a row (lanes 0 / 15 and columns past the image: never stored)
    const int wo = w0 + lr;
    const bool inw = lr >= 1 && lr <= 14 && wo < q.Wout;
    const bool col1 = wo >= 0 && wo < p.Wout;                        // this lane's first-layer column lies inside the image
    const __amdgpu_buffer_rsrc_t ro = make_rsrc((T*)q.out + (size_t)n * q.Hout * q.Wout * q.Cout, q.Hout * q.Wout * q.Cout * (int)sizeof(T));
    const int orow = q.Wout * q.Cout * (int)sizeof(T);
    const int ooff = (inw && lq * 4 < q.Cout) ? (wo * q.Cout + lq * 4) * (int)sizeof(T) : kOob;
    float4 sc1, sh1, sc2, sh2;
    load_affine4(p.scale, p.shift, lq * 4, p.Cout, sc1, sh1);
    load_affine4(q.scale, q.shift, lq * 4, q.Cout, sc2, sh2);
    const bool affine1 = p.scale || p.shift, affine2 = q.scale || q.shift;
    char* ywr = yb + (lr + 1) * 32 + lq * 8;                         // where this lane's 4 couts of pixel lr go
    const char* yrd = yb + lr * 32 + lq * 16;                        // B fragment of column shift kw: + kw * 32 (lq < 2; else zeros)

    // (both layers' weight fragments in registers for the whole strip - 194 VGPRs, two workgroups per CU - were measured: 0.3345 vs 0.3251 s
    // per 8-direction 512^3 prediction with the fragments re-read from LDS every row at four workgroups per CU: not kept)
    // x row hi completes first-layer row r1 = hi - 1, which completes second-layer row r2 = r1 - 1: three accumulators roll per layer
    f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0, a2 = a0, b0 = a0, b1 = a0, b2 = a0;
    uint4 ring[kD][3];
    const int hfirst = h0 - 2, hlast = h1 + 1;                       // x rows this strip needs (rows outside the image load as zeros)
#pragma unroll
    for (int u = 0; u < kD; ++u) load_row(rows, hfirst + u, ring[u]);
    for (int base = hfirst; base <= hlast; base += kD) {
#pragma unroll
        for (int u = 0; u < kD; ++u) {
            const int hi = base + u;
            if (hi > hlast) break;
            row_into3<T, true>(a0, a1, a2, wl1, wbase_l, [&](int kw) { return ring[u][kw]; });
            load_row(rows, hi + kD, ring[u]);
            // ---- first-layer row r1 is complete: epilogue, then into the wave's LDS row (zeros outside the image) ----
            const int r1 = hi - 1;
            {
                float v[4] = {a0[0], a0[1], a0[2], a0[3]};
                if (affine1) affine4(v, sc1, sh1);
                activate4(v, p.relu);
                const bool in1 = col1 && r1 >= 0 && r1 < p.Hout && lq * 4 < Cmid;
                uint2 pk;
                pk.x = in1 ? pack2<T>(v[0], v[1]) : 0u;
                pk.y = in1 ? pack2<T>(v[2], v[3]) : 0u;
                *reinterpret_cast<uint2*>(ywr) = pk;
            }
            roll3(a0, a1, a2);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // the row is in LDS (one wave: its LDS operations execute in order)
            __builtin_amdgcn_wave_barrier();
            // ---- second layer: first-layer row r1 feeds rows r1 + 1 (kh 0), r1 (kh 1), r1 - 1 (kh 2) ----
            // (the fragment as a select, captured by value: written as a conditional load inside the helper the kernel spills at its 128 VGPRs)
            row_into3<T, true>(b0, b1, b2, wl2, wbase_l,
                               [=](int kw) { return lq < 2 ? *reinterpret_cast<const uint4*>(yrd + kw * 32) : make_uint4(0u, 0u, 0u, 0u); });
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // the fragments are in registers before the next row overwrites the LDS row
            __builtin_amdgcn_wave_barrier();
            const int r2 = r1 - 1;                                   // this second-layer row is complete now
            {
                float v[4] = {b0[0], b0[1], b0[2], b0[3]};
                if (affine2) affine4(v, sc2, sh2);
                activate4(v, q.relu);
                store4<T>(ro, (r2 >= h0 && r2 < h1) ? ooff : kOob, r2 * orow, v);
            }
            roll3(b0, b1, b2);
        }
    }
}

// ---- segmentation head: <= 4 classes ---------------------------------------------------------------------------------
// Same strip walk as conv_direct_kernel, but with <= 4 output channels a 16-row MFMA tile would be 3/4 empty and the
// per-pixel epilogue (softmax / arg-max in prediction) would run on lanes that hold nothing: the kernel is VALU-bound.
// So the FOUR output rows h, h+1, h+2, h+3 (h % 4 == 0) share one accumulator tile - row h + q lives in MFMA rows 4q..4q+3,
// i.e. in the lanes of quad q.  An input row hi feeds output rows hi+1 (kh = 0), hi (kh = 1) and hi-1 (kh = 2): the weight
// operand for input-row phase m = hi & 3 carries W[kh = 0] in quad (m+1)&3, W[kh = 1] in quad m, W[kh = 2] in quad (m+3)&3
// and zeros in the fourth quad, so ONE MFMA per kw does what took three (12 phase matrices, built once per workgroup in
// LDS).  A finished row is moved out of its quad with a select; every fourth row all 64 lanes hold one finished pixel each
// and run the epilogue once.  Arithmetic per output value - products, order of accumulation, softmax - is unchanged.
// MODE 2: fp32 NCHW logits + bias (training / plain forward); 3: prediction - no logits leave the kernel: softmax -> first
// arg-max -> fp16 max-prob, cropped and written at the direction's voxel address as label / probability or as a packed key
// through an (order-free) atomic max.
template <typename T, int MODE>
__global__ __launch_bounds__(256, 4) void conv_head_kernel(ConvParams p, DirectGeom g, VolScatter vsc) {
    constexpr int EPS = CT<T>::EPS, kD = 4, NMAT = 12;
    __shared__ __attribute__((aligned(16))) char wl[NMAT * 16 * kPS];
    asm volatile("" ::"s"(p.src0), "s"(p.w), "s"(p.out), "s"(p.C0), "s"(p.Hin), "s"(p.Win), "s"(p.Hout), "s"(p.Wout), "s"(p.Cout),
                 "s"(p.shift), "s"(g.strips_w), "s"(g.chunks_h), "s"(g.RH), "s"(g.sw_magic), "s"(g.ch_magic), "s"(g.nwaves));
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lq = lane >> 4, lr = lane & 15;
    const int Cin = p.C0, K = p.Cout;
    {   // phase matrices: row = (m * 3 + kw) * 16 + 4 * quad + class
        const __amdgpu_buffer_rsrc_t rw = make_rsrc(p.w, K * 9 * Cin * (int)sizeof(T));
#pragma unroll
        for (int i = 0; i < NMAT * 16 * 4 / 256; ++i) {
            const int item = tid + i * 256;
            const int row = item >> 2, seg = item & 3;
            const int mat = row >> 4, quad = (row >> 2) & 3, k = row & 3;
            const int m = mat / 3, kw = mat - m * 3;
            const int kh = quad == ((m + 1) & 3) ? 0 : quad == m ? 1 : quad == ((m + 3) & 3) ? 2 : -1;
            const bool ok = kh >= 0 && k < K && seg * EPS < Cin;
            *reinterpret_cast<uint4*>(wl + swz(row, row, seg)) = bload(rw, ok ? ((k * 9 + kh * 3 + kw) * Cin + seg * EPS) * (int)sizeof(T) : -1, 0);
        }
    }
    __syncthreads();
    const int gw = blockIdx.x * 4 + wave;                   // this wave's strip
    if (gw >= g.nwaves) return;
    const Strip st = strip_of(gw, g);
    const int n = st.n, w0 = st.ws * 16, h0 = st.hc * g.RH, h1 = min(p.Hout, h0 + g.RH);   // RH % 4 == 0: h0 & 3 == 0
    const int h1r = (h1 + 3) & ~3;
    const RowLoader rows = row_loader<T>(p, n, w0, 0, lq, lr);
    const int wbase_l = swz(lr, lr, lq);
    const int wo = w0 + lr;
    const bool inw = wo < p.Wout;
    float bias[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) bias[r] = (p.shift && r < K) ? p.shift[r] : 0.f;
    const int plane = p.Hout * p.Wout * 4;
    const __amdgpu_buffer_rsrc_t ro = MODE == 2 ? make_rsrc((float*)p.out + (size_t)n * K * p.Hout * p.Wout, K * plane) : make_rsrc(nullptr, 0);

    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f}, done = f32x4{0.f, 0.f, 0.f, 0.f};
    uint4 ring[kD][3];
#pragma unroll
    for (int u = 0; u < kD; ++u) load_row(rows, h0 - 1 + u, ring[u]);
    for (int base = h0 - 1; base <= h1r; base += kD) {
#pragma unroll
        for (int u = 0; u < kD; ++u) {
            const int hi = base + u;
            if (hi > h1r) break;
            const int m = (u + 3) & 3;                        // hi & 3 (compile time: base & 3 == 3)
            int wb = wbase_l;
            asm volatile("" : "+v"(wb));                      // phase matrices stay in LDS, not in 48 hoisted registers
#pragma unroll
            for (int kw = 0; kw < 3; ++kw)
                mma16<T>(acc, *reinterpret_cast<const uint4*>(wl + (m * 3 + kw) * 16 * kPS + wb), ring[u][kw]);
            load_row(rows, hi + kD, ring[u]);
            const int qd = (u + 2) & 3;                       // output row hi - 1 is complete; it lives in quad (hi - 1) & 3
            if (lq == qd) { done = acc; acc = f32x4{0.f, 0.f, 0.f, 0.f}; }
            if (qd == 3) {                                    // rows hi-4 .. hi-1 are out: lane (lq, lr) owns row hi-4+lq, column wo
                const int h = hi - 4 + lq;
                const bool live = h >= h0 && h < h1 && inw;
                float v[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = done[r] + bias[r];
                if constexpr (MODE == 2) {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[r]), ro, (live && r < K) ? (h * p.Wout + wo) * 4 : kOob, r * plane, 0);
                } else {                                      // same arithmetic, in the same order, as logits_to_volume_kernel
                    float mx = v[0];
#pragma unroll
                    for (int r = 1; r < 4; ++r) if (r < K) mx = fmaxf(mx, v[r]);
                    float sum = 0.f;
#pragma unroll
                    for (int r = 0; r < 4; ++r) if (r < K) sum += expf(v[r] - mx);
                    float best = -1.f;
                    int lab = 0;
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (r < K) { const float pk = __fdiv_rn(expf(v[r] - mx), sum); if (pk > best) { best = pk; lab = r; } }
                    const int rr = h - vsc.m.crop_top, jj = wo - vsc.m.crop_left;
                    if (live && rr >= 0 && rr < vsc.m.h && jj >= 0 && jj < vsc.m.w) {
                        const int64_t addr = vsc.m.base + (int64_t)(vsc.s0 + n) * vsc.m.ss + (int64_t)rr * vsc.m.sh + (int64_t)jj * vsc.m.sw;
                        const __half hv = __float2half_rn(best);
                        const uint32_t hb = __builtin_bit_cast(uint16_t, hv);
                        if (vsc.mode == 0) {
                            if (vsc.labels) vsc.labels[addr] = (uint8_t)lab;
                            if (vsc.probs) vsc.probs[addr] = (uint16_t)hb;
                        } else if (!vsc.stage) {
                            atomicMax(vsc.keys + addr, (hb << 16) | ((uint32_t)(15 - vsc.direction) << 8) | (uint32_t)lab);
                        } else {   // un-cropped slice layout; launch_keys_stage_scatter does the volume addressing
                            vsc.stage[((int64_t)n * p.Hout + h) * p.Wout + wo] = (hb << 16) | ((uint32_t)(15 - vsc.direction) << 8) | (uint32_t)lab;
                        }
                    }
                }
            }
        }
    }
}

// ---- host: geometry and launchers -------------------------------------------------------------------------------------------
// N images of H x W output pixels as strips of `cols` columns and chunks of RH rows, RH a multiple of `row_mult` (2: the walk
// of an accumulator per row; 4: the head's four rows per accumulator tile).  Rows per wave: every wave pays a 2-row warm-up of
// its input ring; with >= 4 Mi output pixels per launch (px: prediction batches of 512 x 512 slices) there are waves to spare
// and longer strips win (512^3 x 12 prediction: 32 rows 0.507 s, 128 rows 0.499 s).
// Measured, not kept: an XCD-local strip order (common.h: xcd_block; 0.5207 vs 0.5212 s per 512^3 x 12 prediction); fewer
// workgroups per CU, enforced with unused dynamic LDS (the prediction at 2 / 3 per CU 0.559 / 0.542 s against 0.524 s at the
// kernels' own limit of 4).
static DirectGeom strip_geom(int N, int H, int W, int cols, int row_mult, long px) {
    DirectGeom g{};
    g.strips_w = cdiv(W, cols);
    const bool big = px >= (4L << 20) * 4;
    g.RH = std::max(row_mult, vs_option(big ? "conv_direct_rows_big" : "conv_direct_rows") & ~(row_mult - 1));
    g.chunks_h = cdiv(H, g.RH);
    g.sw_magic = 0xffffffffu / (unsigned)g.strips_w + 1u;
    g.ch_magic = 0xffffffffu / (unsigned)g.chunks_h + 1u;
    g.nwaves = N * g.strips_w * g.chunks_h;
    return g;
}
// conv_direct_kernel's geometry: one statistics row per wave (conv_plan's stat_rows)
static DirectGeom direct_geom(const ConvParams& p, int row_mult = 2) {
    return strip_geom(p.N, p.Hout, p.Wout, 16, row_mult, (long)p.N * p.Hout * p.Wout);
}

// p.out_f32 holds the fp32 bit alone here; the layout bit arrives as out_nchw
template <typename T>
int launch_direct(const ConvParams& p, int out_nchw, hipStream_t s) {
    const bool head = p.scatter || (p.Cout & 3) != 0 || out_nchw;
    const DirectGeom g = direct_geom(p, head ? 4 : 2);   // the head's four output rows per accumulator tile: strips start at multiples of 4
    VS_REQUIRE((double)p.Hin * p.Win * p.C0 * sizeof(T) < 2.0e9 && (long)g.nwaves * 16 < (1L << 32), "conv_direct: tensor too large");
    if (head) VS_REQUIRE(!p.up0 && !p.relu && !p.scale && !p.stats_partial, "conv_head: plain 3x3 head only");
    const dim3 grid(cdiv(g.nwaves, 4));
    VolScatter sc{};
    if (p.scatter) {
        sc = *p.scatter;
        ConvParams q = p;
        q.scatter = nullptr;
        hipLaunchKernelGGL((conv_head_kernel<T, 3>), grid, dim3(256), 0, s, q, g, sc);
    } else if (head) {
        VS_REQUIRE(out_nchw && p.Cout <= 4 && !p.pool0 && !p.scale, "conv_direct: unsupported ragged output");
        hipLaunchKernelGGL((conv_head_kernel<T, 2>), grid, dim3(256), 0, s, p, g, sc);
    } else if (p.pool0) {
        hipLaunchKernelGGL((conv_direct_kernel<T, 1>), grid, dim3(256), 0, s, p, g);
    } else {
        VS_REQUIRE(!p.out_f32, "conv_direct: fp32 NHWC output is not supported");
        hipLaunchKernelGGL((conv_direct_kernel<T, 0>), grid, dim3(256), 0, s, p, g);
    }
    VS_LAUNCH_CHECK();
    return VS_OK;
}

// conv_direct_pair_kernel: strips of 14 columns of the second layer's output (the caller has asked conv_pair_ok)
static int launch_pair(int dtype, const ConvParams& p, const ConvParams& q, hipStream_t s) {
    const DirectGeom g = strip_geom(q.N, q.Hout, q.Wout, 14, 2, (long)q.N * q.Hout * q.Wout);
    VS_REQUIRE((long)g.nwaves * 16 < (1L << 32), "conv_pair: grid too large");
    const dim3 grid(cdiv(g.nwaves, 4));
    if (dtype == VS_BF16) hipLaunchKernelGGL((conv_direct_pair_kernel<bf16_t>), grid, dim3(256), 0, s, p, q, g);
    else hipLaunchKernelGGL((conv_direct_pair_kernel<f16_t>), grid, dim3(256), 0, s, p, q, g);
    VS_LAUNCH_CHECK();
    return VS_OK;
}

// head_dgrad_planes_kernel (the caller has asked head_dgrad_planes_ok); always the short strips of a training launch
static int launch_head_dgrad(int dtype, const float* dl, const void* w, void* out, int N, int classes, int H, int W, int C, hipStream_t s) {
    const DirectGeom g = strip_geom(N, H, W, 16, 2, 0);
    const dim3 grid(cdiv(g.nwaves, 4));
    const bool two = 9 * classes > 32;
    if (dtype == VS_BF16) {
        if (two) hipLaunchKernelGGL((head_dgrad_planes_kernel<bf16_t, 2>), grid, dim3(256), 0, s, dl, (const bf16_t*)w, (bf16_t*)out, N, classes, H, W, C, g);
        else hipLaunchKernelGGL((head_dgrad_planes_kernel<bf16_t, 1>), grid, dim3(256), 0, s, dl, (const bf16_t*)w, (bf16_t*)out, N, classes, H, W, C, g);
    } else {
        if (two) hipLaunchKernelGGL((head_dgrad_planes_kernel<f16_t, 2>), grid, dim3(256), 0, s, dl, (const f16_t*)w, (f16_t*)out, N, classes, H, W, C, g);
        else hipLaunchKernelGGL((head_dgrad_planes_kernel<f16_t, 1>), grid, dim3(256), 0, s, dl, (const f16_t*)w, (f16_t*)out, N, classes, H, W, C, g);
    }
    VS_LAUNCH_CHECK();
    return VS_OK;
}

}  // namespace strip
