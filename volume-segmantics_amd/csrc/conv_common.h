// Pieces shared by the convolution kernel families: the chunk constants and mma16 (tile kernel of conv_igemm.hip, conv_ring.h,
// conv_stream.h, the strip kernels of conv_strip.h), and conv_epilogue, the epilogue of the tile and ring kernels (the strip
// kernels have their own).
#pragma once
#include <type_traits>

#include "common.h"

template <typename T> struct CT;
template <> struct CT<bf16_t> { static constexpr int CK = 32, EPS = 8; };
template <> struct CT<f16_t> { static constexpr int CK = 32, EPS = 8; };
template <> struct CT<float> { static constexpr int CK = 16, EPS = 4; };

// value as it reads back after being stored in T
template <typename T>
__device__ __forceinline__ float4 ld4_roundtrip(const float (&v)[4]) {
    if constexpr (sizeof(T) == 2) {
        const float a[4] = {v[0], v[1], v[2], v[3]};
        T t[4];
        for (int i = 0; i < 4; ++i) Elem<T>::st(t + i, a[i]);
        return make_float4(Elem<T>::ld(t), Elem<T>::ld(t + 1), Elem<T>::ld(t + 2), Elem<T>::ld(t + 3));
    } else
        return make_float4(v[0], v[1], v[2], v[3]);
}

// the compiler's wait for a value that a load is still bringing in happens HERE (and not at its first use)
__device__ __forceinline__ void landed(const uint2& v) { asm volatile("" ::"v"(v.x), "v"(v.y)); }
__device__ __forceinline__ void landed(const float4& v) { asm volatile("" ::"v"(v.x), "v"(v.y), "v"(v.z), "v"(v.w)); }
__device__ __forceinline__ void landed(const f16raw4& v) { landed(v.u); }

template <typename T>
__device__ __forceinline__ void mma16(f32x4& acc, const uint4& a, const uint4& b) {
    if constexpr (std::is_same<T, f16_t>::value) {
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), acc, 0, 0, 0);
    } else if constexpr (sizeof(T) == 2) {
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b),
                                                      acc, 0, 0, 0);
    } else {
        // lane (l>>4)=q holds channels 4q..4q+3 of the chunk for both operands: step s pairs element s
        const float4 fa = __builtin_bit_cast(float4, a), fb = __builtin_bit_cast(float4, b);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(fa.x, fb.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(fa.y, fb.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(fa.z, fb.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(fa.w, fb.w, acc, 0, 0, 0);
    }
}


// Epilogue of an implicit-GEMM tile: lane (lq, lr) of wave `wave` holds, for pixel tile i and cout tile j, the 4 output
// channels n0 + 16j + 4lq .. +3 of pixel  wave*PT*16 + 16i + lr  of the TH x TW patch at (n, h0, w0).
// Optional: per-channel sum / sum-of-squares partials of the raw accumulators (row `tile` of p.stats_partial), fused
// affine + residual + ReLU, split output (dgrad through a concat), 2x2 sum-pool (dgrad through nearest x2 upsampling),
// fp32 / NCHW stores (segmentation head).  `smem` must provide 6*NW*BN floats (2*NW*BN of partials, and in the BN-backward form a
// 4*BN table per wave) that are free once every wave has arrived: less than the staged tiles of any instantiation.
template <typename T, int BN, int PT, int NW = 4>
__device__ __forceinline__ void conv_epilogue(const ConvParams& p, int tw_shift, int out_nchw, int n, int h0, int w0, int n0,
                                              int tile, f32x4 (&acc)[PT][BN / 16], char* smem) {
    constexpr int NJ = BN / 16;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lq = lane >> 4, lr = lane & 15;
    const int TW = 1 << tw_shift;
    struct { int tw_shift, out_nchw; } g{tw_shift, out_nchw};
    // ---- epilogue: lane holds pixel (lr) x couts 4*lq..4*lq+3 of each 16x16 tile ----
    const bool ragged = (p.Cout & 3) != 0 || g.out_nchw;  // segmentation head only
    // The register-staged kernels arrive with the prefetch of a chunk that does not exist still counted (issued a whole chunk ago,
    // never read).  Retire it here, where it costs nothing: the compiler would otherwise wait for it wherever its registers are
    // used next - between the output stores, where the same wait also covers the stores in front of it.
    __builtin_amdgcn_s_waitcnt(0x0f70);                   // vmcnt(0) alone
    // (1) optional per-channel statistics of the raw accumulators (train-mode BN of the bf16 path)
    if (p.stats_partial || p.stats_bins) {
        float* red = reinterpret_cast<float*>(smem);  // [NW waves][2][BN]
        __syncthreads();                               // staged tiles are dead
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int i = 0; i < PT; ++i) {
                const int pl = wave * (PT * 16) + i * 16 + lr;
                const bool ok = h0 + (pl >> g.tw_shift) < p.Hout && w0 + (pl & (TW - 1)) < p.Wout;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float x = ok ? acc[i][j][r] : 0.f;
                    s1[r] += x; s2[r] += x * x;
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) { s1[r] += __shfl_xor(s1[r], o, 64); s2[r] += __shfl_xor(s2[r], o, 64); }
            }
            if (lr == 0) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    red[(wave * 2 + 0) * BN + j * 16 + lq * 4 + r] = s1[r];
                    red[(wave * 2 + 1) * BN + j * 16 + lq * 4 + r] = s2[r];
                }
            }
        }
        __syncthreads();
        if (tid < 2 * BN) {
            const int k = tid / BN, cc = tid % BN;
            if (n0 + cc < p.Cout) {
                float a = 0.f;
#pragma unroll
                for (int w = 0; w < NW; ++w) a += red[(w * 2 + k) * BN + cc];
                if (p.stats_bins)      // fixed point: the order the workgroups arrive in cannot change the total
                    atomicAdd(p.stats_bins + ((size_t)(tile & (p.stats_nb - 1)) * 2 + k) * p.Cout + n0 + cc,
                              (unsigned long long)__double2ll_rn((double)a * (k ? kStatScale2 : kStatScale1)));
                else
                    p.stats_partial[((size_t)tile * 2 + k) * p.Cout + n0 + cc] = a;
            }
        }
    }
    // (1b) dgrad that completes the gradient of a conv+BN(+ReLU) unit's activation: mask, store g, BN-backward partials
    if (p.bz) {
        float* red = reinterpret_cast<float*>(smem);  // [NW waves][2][BN]
        float* par = red + (NW * 2 + wave * 4) * BN;   // this wave's own [4][BN]: mean, invstd, invstd * gamma, beta of the cout tile
        __syncthreads();                               // staged tiles are dead
        // EVERY global load of the epilogue is issued here, in front of the first store: the per-channel vectors of the whole cout
        // tile (lane l of each wave fetches channel n0 + l; they reach the lanes that use them through the wave's LDS table), then
        // residual (= earlier contributions to this gradient), z and y of all PT x NJ sub-tiles.  Issued back to back they cost one
        // memory round trip; a load issued behind a store waits for that store's acknowledgement as well.  None of them may fault
        // on a lane the stores skip (ragged tiles, cout tail): such a lane reads the tensor's first elements instead (channel
        // Cout - 1 for the vectors) and the value is never used.
        const bool affine = p.brelu && !p.by;
        float pm = 0.f, pi = 0.f, pg = 0.f, pb = 0.f;
        if (BN == 64 || lane < BN) {
            const int cp = min(n0 + lane, p.Cout - 1);
            pm = p.bmean[cp]; pi = p.binvstd[cp];
            if (affine) { pg = p.bgamma[cp]; pb = p.bbeta[cp]; }
        }
        typename Raw4<T>::type rv[PT][NJ], zq[PT][NJ], yq[PT][NJ];
        size_t off[PT][NJ];
        bool live[PT][NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int c = n0 + j * 16 + lq * 4;
#pragma unroll
            for (int i = 0; i < PT; ++i) {
                const int pl = wave * (PT * 16) + i * 16 + lr;
                const int ho = h0 + (pl >> g.tw_shift), wo = w0 + (pl & (TW - 1));
                live[i][j] = ho < p.Hout && wo < p.Wout && c < p.Cout;
                off[i][j] = (((size_t)n * p.Hout + ho) * p.Wout + wo) * p.Cout + c;
                const size_t lo = live[i][j] ? off[i][j] : (size_t)0;
                rv[i][j] = yq[i][j] = typename Raw4<T>::type{};
                if (p.residual) rv[i][j] = ld4raw((const T*)p.residual + lo);
                zq[i][j] = ld4raw((const T*)p.bz + lo);
                if (p.brelu && p.by) yq[i][j] = ld4raw((const T*)p.by + lo);
            }
        }
        // ONE wait for all of them: no load is pending once the stores begin, so no later wait can include a store's
        // acknowledgement (left to itself the compiler waits per sub-tile, and behind the conditional stores it counts as if
        // none had been issued)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int i = 0; i < PT; ++i) {
                landed(zq[i][j]);
                if (p.residual) landed(rv[i][j]);
                if (p.brelu && p.by) landed(yq[i][j]);
            }
        if (BN == 64 || lane < BN) {
            par[lane] = pm; par[BN + lane] = pi;
            if (affine) { par[2 * BN + lane] = pi * pg; par[3 * BN + lane] = pb; }
        }
        __builtin_amdgcn_wave_barrier();               // the table is read by the wave that wrote it: program order is enough
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
            float ga[4] = {0.f, 0.f, 0.f, 0.f}, be[4] = {0.f, 0.f, 0.f, 0.f};
            const float4 m4 = *reinterpret_cast<const float4*>(par + j * 16 + lq * 4), i4 = *reinterpret_cast<const float4*>(par + BN + j * 16 + lq * 4);
            const float mu[4] = {m4.x, m4.y, m4.z, m4.w}, is[4] = {i4.x, i4.y, i4.z, i4.w};
            if (affine) {
                const float4 g4 = *reinterpret_cast<const float4*>(par + 2 * BN + j * 16 + lq * 4), b4 = *reinterpret_cast<const float4*>(par + 3 * BN + j * 16 + lq * 4);
                ga[0] = g4.x; ga[1] = g4.y; ga[2] = g4.z; ga[3] = g4.w;
                be[0] = b4.x; be[1] = b4.y; be[2] = b4.z; be[3] = b4.w;
            }
#pragma unroll
            for (int i = 0; i < PT; ++i) {
                if (!live[i][j]) continue;
                const float4 r4 = unpack4(rv[i][j]), z4 = unpack4(zq[i][j]), y4 = unpack4(yq[i][j]);
                float v[4] = {acc[i][j][0] + r4.x, acc[i][j][1] + r4.y, acc[i][j][2] + r4.z, acc[i][j][3] + r4.w};
                const float zv[4] = {z4.x, z4.y, z4.z, z4.w};
                if (p.brelu) {
                    if (p.by) {
                        v[0] = y4.x > 0.f ? v[0] : 0.f; v[1] = y4.y > 0.f ? v[1] : 0.f;
                        v[2] = y4.z > 0.f ? v[2] : 0.f; v[3] = y4.w > 0.f ? v[3] : 0.f;
                    } else {
#pragma unroll
                        for (int r = 0; r < 4; ++r) v[r] = ((zv[r] - mu[r]) * ga[r] + be[r]) > 0.f ? v[r] : 0.f;
                    }
                }
                st4((T*)p.out + off[i][j], make_float4(v[0], v[1], v[2], v[3]));
                const float4 gq = ld4_roundtrip<T>(v);   // the statistics see exactly what was stored
                const float gv[4] = {gq.x, gq.y, gq.z, gq.w};
#pragma unroll
                for (int r = 0; r < 4; ++r) { s1[r] += gv[r]; s2[r] += gv[r] * (zv[r] - mu[r]) * is[r]; }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) { s1[r] += __shfl_xor(s1[r], o, 64); s2[r] += __shfl_xor(s2[r], o, 64); }
            }
            if (lr == 0) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    red[(wave * 2 + 0) * BN + j * 16 + lq * 4 + r] = s1[r];
                    red[(wave * 2 + 1) * BN + j * 16 + lq * 4 + r] = s2[r];
                }
            }
        }
        __syncthreads();
        if (tid < 2 * BN) {
            const int k = tid / BN, cc = tid % BN;
            if (n0 + cc < p.Cout) {
                float a = 0.f;
#pragma unroll
                for (int w = 0; w < NW; ++w) a += red[(w * 2 + k) * BN + cc];
                p.bstats_partial[((size_t)tile * 2 + k) * p.Cout + n0 + cc] = a;
            }
        }
        return;
    }
    // (2) outputs
    const int pool_c = p.pool0 ? (p.out1 ? p.split_c : p.Cout) : 0;
    // Every global load of the vector path - scale / shift of all NJ cout sub-tiles, residual of all PT x NJ sub-tiles - in front of
    // the first store, for the reason given at (1b), and ONE wait for all of them: no load is pending once the stores begin, so no
    // later wait can include a store's acknowledgement.  The loads sit under ONE uniform test (is there any of the three?) and are
    // straight-line code behind it: a kind that is absent reads the first 16 bytes of the weights instead, a lane the stores skip
    // the first elements of its tensor; neither value is used.  (A test per kind and element makes the compiler wait between the
    // loads, and a wait it cannot pair with its loads comes back behind the stores.)  A launch without any of them - the training
    // forwards - issues no load.
    float4 sc4[NJ], sh4[NJ];
    typename Raw4<T>::type rq[PT][NJ];
    if (!ragged && (p.scale || p.shift || p.residual)) {
        const float* scp = p.scale ? p.scale : (const float*)p.w;
        const float* shp = p.shift ? p.shift : (const float*)p.w;
        const T* rp = p.residual ? (const T*)p.residual : (const T*)p.w;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int c = n0 + j * 16 + lq * 4;
            const int cl = c < p.Cout ? c : 0;
            sc4[j] = *reinterpret_cast<const float4*>(scp + (p.scale ? cl : 0));
            sh4[j] = *reinterpret_cast<const float4*>(shp + (p.shift ? cl : 0));
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int c = n0 + j * 16 + lq * 4;
#pragma unroll
            for (int i = 0; i < PT; ++i) {
                const int pl = wave * (PT * 16) + i * 16 + lr;
                const int ho = h0 + (pl >> g.tw_shift), wo = w0 + (pl & (TW - 1));
                const bool to_out = !p.out1 || c < p.split_c;       // the residual belongs to `out`
                const bool use = p.residual && ho < p.Hout && wo < p.Wout && c < p.Cout && !(PT >= 2 && c < pool_c) && to_out;
                const size_t o = (((size_t)n * p.Hout + ho) * p.Wout + wo) * (p.out1 ? p.split_c : p.Cout) + c;
                rq[i][j] = ld4raw(rp + (use ? o : (size_t)0));
            }
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            landed(sc4[j]); landed(sh4[j]);
#pragma unroll
            for (int i = 0; i < PT; ++i) landed(rq[i][j]);
        }
    }
    // the stores: `ragged` is uniform, so the two forms are two instances of the loops and not a test per element
    auto outputs = [&](auto ragged_) {
        constexpr bool kRagged = decltype(ragged_)::value;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int c = n0 + j * 16 + lq * 4;
            if (PT >= 2 && c < pool_c) {
                // dgrad through nearest-x2 upsampling: sum the 2x2 block (rows i, i+1 of this wave; lanes lr, lr^1)
                if constexpr (PT >= 2) {
#pragma unroll
                    for (int ip = 0; ip < PT / 2; ++ip) {
                        float v[4];
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            v[r] = acc[2 * ip][j][r] + acc[2 * ip + 1][j][r];
                            v[r] += __shfl_xor(v[r], 1, 64);
                        }
                        const int ho = h0 + wave * PT + 2 * ip, wo = w0 + lr;
                        if ((lr & 1) == 0 && ho < p.Hout && wo < p.Wout && c < p.Cout) {
                            const size_t o = (((size_t)n * (p.Hout >> 1) + (ho >> 1)) * (p.Wout >> 1) + (wo >> 1)) * pool_c + c;
                            st4((T*)p.out + o, make_float4(v[0], v[1], v[2], v[3]));
                        }
                    }
                }
                continue;
            }
#pragma unroll
            for (int i = 0; i < PT; ++i) {
                const int pl = wave * (PT * 16) + i * 16 + lr;
                const int ho = h0 + (pl >> g.tw_shift), wo = w0 + (pl & (TW - 1));
                if (ho >= p.Hout || wo >= p.Wout || c >= p.Cout) continue;
                const size_t pix = ((size_t)n * p.Hout + ho) * p.Wout + wo;
                float v[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
                if constexpr (!kRagged) {
                    if (p.scale) {
                        const float4 sc = sc4[j], sh = sh4[j];
                        v[0] = v[0] * sc.x + sh.x; v[1] = v[1] * sc.y + sh.y; v[2] = v[2] * sc.z + sh.z; v[3] = v[3] * sc.w + sh.w;
                    } else if (p.shift) {
                        const float4 sh = sh4[j];
                        v[0] += sh.x; v[1] += sh.y; v[2] += sh.z; v[3] += sh.w;
                    }
                    // destination (possibly split across two tensors: dgrad through a channel concat)
                    char* dst = (char*)p.out;
                    int cd = c, cstride = p.Cout;
                    if (p.out1) {
                        if (c >= p.split_c) { dst = (char*)p.out1; cd = c - p.split_c; cstride = p.Cout - p.split_c; }
                        else cstride = p.split_c;
                    }
                    const size_t o = pix * cstride + cd;
                    if (p.residual && dst == (char*)p.out) {
                        const float4 rv = unpack4(rq[i][j]);
                        v[0] += rv.x; v[1] += rv.y; v[2] += rv.z; v[3] += rv.w;
                    }
                    if (p.relu == 1) { v[0] = fmaxf(v[0], 0.f); v[1] = fmaxf(v[1], 0.f); v[2] = fmaxf(v[2], 0.f); v[3] = fmaxf(v[3], 0.f); }
                    else if (p.relu == 2) {      // swish (evaluation-mode EfficientNet: BatchNorm folded into scale / shift, then x * sigmoid(x))
#pragma unroll
                        for (int r = 0; r < 4; ++r) v[r] = v[r] / (1.f + __expf(-v[r]));
                    }
                    if (p.out_f32) st4((float*)dst + o, make_float4(v[0], v[1], v[2], v[3]));
                    else st4((T*)dst + o, make_float4(v[0], v[1], v[2], v[3]));
                } else {      // (segmentation head: element by element, its few loads between its stores)
                    const int nv = min(4, p.Cout - c);
                    for (int r = 0; r < nv; ++r) {
                        float x = v[r];
                        if (p.scale) x = x * p.scale[c + r] + p.shift[c + r];
                        else if (p.shift) x += p.shift[c + r];
                        if (p.residual) x += Elem<T>::ld((const T*)p.residual + pix * p.Cout + c + r);
                        if (p.relu == 1) x = fmaxf(x, 0.f);
                        else if (p.relu == 2) x = x / (1.f + __expf(-x));
                        if (g.out_nchw) ((float*)p.out)[(((size_t)n * p.Cout + c + r) * p.Hout + ho) * p.Wout + wo] = x;
                        else if (p.out_f32) ((float*)p.out)[pix * p.Cout + c + r] = x;
                        else Elem<T>::st((T*)p.out + pix * p.Cout + c + r, x);
                    }
                }
            }
        }
    };
    if (ragged) outputs(std::true_type{});
    else outputs(std::false_type{});
}
