// Implicit-GEMM NHWC convolution on MFMA (gfx950), im2col-free: the LDS-staged tile kernel, and the plan and dispatch of
// every convolution kernel family.
//
// conv_igemm_kernel - the general one.  A workgroup (8 waves on 16x16-pixel tiles; 4 waves on 8x16 / 8x8 tiles for small
// images and stride 2) computes a tile of output pixels of one image times BN (64 / 32 / 16) output channels.  For every
// chunk of CK input channels (64 bytes per pixel: 32 bf16 / 16 f32) the input halo patch and the BN x taps weight slab are
// staged in LDS once and reused by all KH*KW taps: a tap is a constant byte offset into the staged patch, so there is no
// im2col buffer anywhere.  MFMA orientation: A = weights (rows = cout), B = pixels (cols), so each lane ends up with 4
// consecutive output channels of one pixel -> 8/16-byte NHWC stores.
//   * staging: raw buffer loads (one descriptor per image, 32-bit lane offsets, offset -1 -> zeros) issued one or two chunks
//     ahead into registers, written to LDS between two barriers; compile-time tile geometry for stride 1;
//   * LDS: unpadded 64-byte rows, 16-byte segments XOR-swizzled by the patch column (conflict-free ds_read_b128);
//   * 32-wide tiles: fragments of tap t+1 are read while the MFMAs of tap t run, pinned with sched_group_barrier;
//   * workgroup -> tile map is XCD-aware: cout tiles sharing an input patch run back to back on one XCD's L2;
//   * epilogue (conv_common.h): BN-statistics partials, affine, residual, ReLU, split output, 2x2 sum-pool, fp32 / NCHW.
//
// The strip-walk kernels (conv_direct_kernel, conv_head_kernel, conv_direct_pair_kernel, head_dgrad_planes_kernel) - the
// HBM-bound shallow layers (<= 16 couts, Cin within one chunk, large images), the segmentation head and its data gradient,
// every wave walking down a 16-pixel-wide strip with a ring of input rows held in registers - live in conv_strip.h with
// their geometry and launchers, as the ring and stream kernels live in conv_ring.h / conv_stream.h; conv_plan below decides
// which launches they get.
//
// bf16: v_mfma_f32_16x16x32_bf16 (one per 32-channel chunk-tap); f32: 4 x v_mfma_f32_16x16x4_f32 on the same 16-byte
// fragments (exact fp32 FMA chain - the parity path).
//
// Serves every 3x3 / 1x1 convolution of smp.Unet(resnet34) forward (reference call sites vol_seg_2d_trainer.py:424,
// vol_seg_2d_predictor.py:44), with the decoder's nearest-x2 upsample + concat folded into the patch loader, and - fed with
// flipped/transposed weights - their dgrad.
#include <hip/hip_fp16.h>

#include <algorithm>
#include <cstdlib>

#include "conv_common.h"
#include "conv_stream.h"
#include "conv_strip.h"
#include "prof.h"

namespace {

using strip::kPS;   // the staged LDS rows and their swizzle: conv_strip.h
using strip::swz;

struct TileGeom {
    int tw_shift;  // TW = 1 << tw_shift (8 or 16)
    int TH;
    int tiles_h, tiles_w;
    int PH, PW;  // staged patch dims
    int out_nchw;
    unsigned pw_magic, tw_magic;  // x / PW == umulhi(x, pw_magic), x / tiles_w == umulhi(x, tw_magic) for x < 65536
    int groups, ctiles;           // pixel tiles over the whole batch, cout tiles (see the workgroup -> tile map in the kernel)
    unsigned ct_magic, ti_magic;  // x / ctiles, x / (tiles_h * tiles_w)
    unsigned long long* probe;  // phase timestamps (tools/conv_probe.py); null in normal operation
};

// 16-byte patch items per thread (NW = waves per workgroup; the tile has NW*PT*16 pixels)
constexpr int patch_items(int pt, int stride, int nw = 4) {
    return nw == 8 ? 3 : (stride == 2 ? (pt == 2 ? 9 : 5) : (pt == 4 ? 6 : (pt == 2 ? 3 : 2)));
}

// DIL: dilation of a 3x3 kernel (1 or 2; torchvision / smp "replace stride with dilation" stages).  Dilated variants take their
// tile geometry from the launch like the stride-2 ones and use the same staging budget (the patch is (tile + 2 DIL) wide).
// NLOAD: src0 is the PRE-norm output z of the conv -> BN -> ReLU unit in front (ConvParams::nl_*).  The prologue sums the unit's
// statistics bins (every workgroup for itself; workgroup 0 publishes), the chunks are normalised in registers on their way to LDS -
// y = max((z - mean) * (invstd * gamma) + beta, 0) rounded to bf16, the value the normalisation sweep would have stored, zero
// padding left zero - and the workgroups of the first cout tile store the normalised interior of their patch (the activation the
// weight gradient reads later): no normalisation sweep, no launch between the two convolutions.
template <typename T, int BN, int PT, int NTAPS, int STRIDE, int NW = 4, int DIL = 1, bool NLOAD = false>
__global__ __launch_bounds__(NW * 64, NW == 8 ? 4 : 1) void conv_igemm_kernel(ConvParams p, TileGeom g) {
    constexpr int NT = NW * 64;
    constexpr int CK = CT<T>::CK, EPS = CT<T>::EPS;
    constexpr int NJ = BN / 16, KW = NTAPS == 9 ? 3 : 1;
    constexpr int PITEMS = patch_items(PT, DIL > 1 ? 2 : STRIDE, NW);
    constexpr int WROWS = NT / 4;                 // weight rows one pass of the workgroup stages
    constexpr int TS = WROWS / BN;                // taps per pass
    static_assert(WROWS % BN == 0, "cout tile must divide the rows of a staging pass");
    constexpr int WITEMS = (NTAPS + TS - 1) / TS;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lq = lane >> 4, lr = lane & 15;
    // stride-1 kernels have a compile-time tile (16 wide; 8 wide for the 64-pixel tiles of small images), so patch
    // row offsets are instruction immediates; stride-2 kernels take it from the launch
    constexpr bool kStatic = STRIDE == 1 && DIL == 1;
    constexpr int kTWS = PT == 1 ? 3 : 4, kTW = 1 << kTWS, kTH = NW * 16 * PT / kTW, kKH = NTAPS == 9 ? 3 : 1;
    const int tw_shift = kStatic ? kTWS : g.tw_shift;
    const int TW = 1 << tw_shift;
    const int PW = kStatic ? kTW - 1 + KW : g.PW;
    const int PH = kStatic ? kTH - 1 + kKH : g.PH;
    const int TH = kStatic ? kTH : g.TH;
    const int Cin = p.C0 + p.C1;
    const int P = PH * PW;
    char* patch = smem;
    char* wl = smem + P * kPS;
    // pull every kernel argument the prologue needs into SGPRs with ONE batch of scalar loads: left to itself the compiler
    // loads them where first used, a chain of four dependent ~0.3 us round trips at the head of every workgroup
    asm volatile("" ::"s"(p.src0), "s"(p.src1), "s"(p.w), "s"(p.out), "s"(p.C0), "s"(p.C1), "s"(p.up0), "s"(p.Hin), "s"(p.Win),
                 "s"(p.Hout), "s"(p.Wout), "s"(p.pad), "s"(p.Cout), "s"(g.tiles_w), "s"(g.tw_magic), "s"(g.pw_magic), "s"(g.PW),
                 "s"(g.PH), "s"(g.tw_shift), "s"(g.probe), "s"(p.gc));
    unsigned long long tprobe[5];
    if (g.probe) tprobe[0] = wall_clock64();

    // Workgroup -> tile, XCD-aware: consecutive workgroup ids go round-robin to the 8 XCDs (each with its own L2), so the
    // cout tiles that share one input patch are given ids 8 apart - they run back to back on ONE XCD and the patch comes
    // from HBM once (ids differing only in the low 3 bits take different pixel tiles).  With the cout tile as the slow
    // index every XCD would fetch every image: ~2x the traffic in the 256-/512-channel layers (rocprofv3 FETCH_SIZE).
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int gl = g.ctiles == 1 ? slot : (int)__umulhi((unsigned)slot, g.ct_magic);
    const int ytile = slot - gl * g.ctiles;
    const int grp = gl * 8 + xcd;                     // pixel tile index over the whole batch
    if (grp >= g.groups) return;                      // padding of the last round (uniform per workgroup)
    const int tiles_img = g.tiles_h * g.tiles_w;
    const int n = tiles_img == 1 ? grp : (int)__umulhi((unsigned)grp, g.ti_magic);
    const int timg = grp - n * tiles_img;
    const int ty = g.tiles_w == 1 ? timg : (int)__umulhi((unsigned)timg, g.tw_magic);
    const int tx = timg - ty * g.tiles_w;
    const int h0 = ty * TH, w0 = tx * TW;
    const int n0 = ytile * BN;
    const int hbase = h0 * STRIDE - p.pad, wbase = w0 * STRIDE - p.pad;
    // up0: 0 = plain source, 1 = nearest x2 upsampling of a half-resolution source, 2 = the same addressing with zeros at
    // the odd rows / columns (zero stuffing: data gradient of a stride-2 convolution, never materialised)
    const int ush = p.up0 ? 1 : 0;
    const bool stuffed = p.up0 == 2;
    const int H0 = p.Hin >> ush, W0 = p.Win >> ush;
    // Staging loads are raw buffer loads: one descriptor per source (base = this image, so per-lane offsets are 32-bit
    // byte offsets), the chunk's channel offset rides in the scalar offset, and offset -1 (out of range) returns zeros -
    // zero padding, ragged tiles and channel tails cost no branches.
    const __amdgpu_buffer_rsrc_t r0 = __builtin_amdgcn_make_buffer_rsrc(
        (void*)((const T*)p.src0 + (size_t)n * H0 * W0 * p.C0), 0, H0 * W0 * p.C0 * (int)sizeof(T), 0x00020000);
    const __amdgpu_buffer_rsrc_t r1 = __builtin_amdgcn_make_buffer_rsrc(
        (void*)((const T*)p.src1 + (size_t)n * p.Hin * p.Win * p.C1), 0, p.src1 ? p.Hin * p.Win * p.C1 * (int)sizeof(T) : 0, 0x00020000);
    // Grouped convolution (p.gc = 32, BN = 32): the cout tile IS one 32-channel super-group, whose outputs read only the
    // super-group's own 32 input channels: the chunk loop covers [n0, n0 + 32) and the weight rows are 32 channels long
    // (groups narrower than 32 channels are block-diagonal inside the super-group's 32 x 32 slab, zeros elsewhere).
    const int kbeg = p.gc ? n0 : 0, kend = p.gc ? n0 + p.gc : Cin;
    const int CinW = p.gc ? p.gc : Cin;
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)p.w, 0, p.Cout * NTAPS * CinW * (int)sizeof(T), 0x00020000);
    const int dummy = (P + NTAPS * BN) * kPS;    // 64 spare bytes behind the staged tiles: target of the stores of idle items
    // NLOAD: [3][C0 rounded up to 32] floats behind them - mean, invstd * gamma, beta of src0's channels
    float* cst = reinterpret_cast<float*>(smem + dummy + 64);
    const int C0r = (p.C0 + 31) & ~31;
    if constexpr (NLOAD) {
        const long long* bins = reinterpret_cast<const long long*>(p.nl_bins);     // [nl_nb][2][C0]: sum z * 2^24, sum z^2 * 2^16
        const double rows = (double)p.nl_rows;
        for (int ch = tid; ch < p.C0; ch += NT) {
            long long sv = 0, qv = 0;
#pragma unroll 8
            for (int r = 0; r < p.nl_nb; ++r) { sv += bins[((size_t)r * 2 + 0) * p.C0 + ch]; qv += bins[((size_t)r * 2 + 1) * p.C0 + ch]; }
            // (the arithmetic of bn_apply_inline_kernel<T, true>: the same bits as the sweep's statistics)
            const double mu = ((double)sv * (1.0 / kStatScale1)) / rows;
            double var = ((double)qv * (1.0 / kStatScale2)) / rows - mu * mu;
            if (var < 0.0) var = 0.0;
            const float is = (float)(1.0 / sqrt(var + (double)p.nl_eps));
            cst[ch] = (float)mu;
            cst[C0r + ch] = is * p.nl_gamma[ch];
            cst[2 * C0r + ch] = p.nl_beta[ch];
            if (blockIdx.x == 0) {        // one workgroup publishes: statistics for the backward pass, running statistics
                p.nl_mean[ch] = (float)mu;
                p.nl_invstd[ch] = is;
                if (p.nl_rm) {
                    const double unbiased = p.nl_rows > 1 ? var * rows / (double)(p.nl_rows - 1) : var;
                    p.nl_rm[ch] = (float)((1.0 - p.nl_mom) * (double)p.nl_rm[ch] + p.nl_mom * mu);
                    p.nl_rv[ch] = (float)((1.0 - p.nl_mom) * (double)p.nl_rv[ch] + p.nl_mom * unbiased);
                }
            }
        }   // visible to every wave behind the first barrier of the chunk loop
    }

    // ---- chunk-invariant staging addresses (byte offsets; -1 = zero fill) ----
    int poff0[PITEMS], poff1[PITEMS], pdst[PITEMS];
    unsigned ystore = 0;
#pragma unroll
    for (int i = 0; i < PITEMS; ++i) {
        const int item = tid + i * NT;
        const int pp = item >> 2, seg = item & 3;
        const int ph = kStatic ? pp / PW : (int)__umulhi((unsigned)pp, g.pw_magic), pw = pp - ph * PW;
        const int hi = hbase + ph, wi = wbase + pw;
        const bool ok = pp < P && hi >= 0 && hi < p.Hin && wi >= 0 && wi < p.Win;
        poff0[i] = (ok && !(stuffed && ((hi | wi) & 1))) ? (((hi >> ush) * W0 + (wi >> ush)) * p.C0 + seg * EPS) * (int)sizeof(T) : -1;
        poff1[i] = ok ? ((hi * p.Win + wi) * p.C1 + seg * EPS) * (int)sizeof(T) : -1;
        pdst[i] = pp < P ? swz(pp, pw, seg) : dummy;
        if constexpr (NLOAD) {   // items whose normalised value this workgroup stores to nl_y: the tile's own pixels (not the halo), once per source pixel
            const bool mine = ok && hi >= h0 && hi < h0 + TH && wi >= w0 && wi < w0 + TW && !(ush && ((hi | wi) & 1));
            ystore |= mine ? 1u << i : 0u;
        }
    }
    // weight staging: pass i covers rows i*WROWS + (tid >> 2); row = tap*BN + nr, so a pass advances TS taps
    const int wrow0 = tid >> 2, wseg = tid & 3;
    const int wnr = wrow0 % BN, wtap0 = wrow0 / BN;
    const bool wok = n0 + wnr < p.Cout;
    const int woff0 = (((n0 + wnr) * NTAPS + wtap0) * CinW + wseg * EPS) * (int)sizeof(T);
    const int wdst0 = swz(wrow0, wrow0, wseg);   // i*WROWS is a multiple of 16 rows: same swizzle in every pass

    // Prefetch depth: PF chunks are in flight (in registers) while one is being multiplied.  Kernels that run with one or
    // two workgroups per CU and have registers to spare use 2, so a staging load gets two chunk periods to land.
    constexpr int PF = (((NW == 8 && BN <= 32) || (NW == 4 && PT == 1 && STRIDE == 1)) && !(NLOAD && NW == 8)) ? 2 : 1;   // (NLOAD, 8 waves: the second set spills)
    uint4 pregs[PF][PITEMS], wregs[PF][WITEMS];
    auto load_chunk = [&](int c0, uint4 (&preg)[PITEMS], uint4 (&wreg)[WITEMS]) {
        const bool from0 = c0 < p.C0;
        const int cs = from0 ? p.C0 : p.C1;
        const int cb = from0 ? c0 : c0 - p.C0;
        const int nseg = (cs - cb) / EPS;         // valid 16-byte segments of this chunk (< 4 only in a ragged channel tail)
        const int nsegw = (kend - c0) / EPS;
#pragma unroll
        for (int i = 0; i < PITEMS; ++i) {
            int off = from0 ? poff0[i] : poff1[i];
            if (((tid + i * NT) & 3) >= nseg) off = -1;
            preg[i] = from0 ? bload(r0, off, cb * (int)sizeof(T)) : bload(r1, off, cb * (int)sizeof(T));
        }
#pragma unroll
        for (int i = 0; i < WITEMS; ++i) {
            int off = woff0 + i * TS * CinW * (int)sizeof(T);
            if (!wok || wtap0 + i * TS >= NTAPS || wseg >= nsegw) off = -1;
            wreg[i] = bload(rw, off, (c0 - kbeg) * (int)sizeof(T));
        }
    };

    // per-lane LDS read bases: pixel tile i, tap column kw (tap row kh adds the constant kh * PW * kPS)
    int xb[PT][KW];
#pragma unroll
    for (int i = 0; i < PT; ++i) {
        const int pl = wave * (PT * 16) + i * 16 + lr;
        const int th = pl >> tw_shift, tw = pl & (TW - 1);
#pragma unroll
        for (int kw = 0; kw < KW; ++kw) xb[i][kw] = swz((th * STRIDE) * PW + tw * STRIDE + kw * DIL, tw * STRIDE + kw * DIL, lq);
    }
    const int wbase_l = swz(lr, lr, lq);                  // (tap*BN + 16j) is a multiple of 16: it does not change the swizzle
    const int khs = DIL * PW * kPS;

    f32x4 acc[PT][NJ];
#pragma unroll
    for (int i = 0; i < PT; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    load_chunk(kbeg, pregs[0], wregs[0]);
    if (PF == 2 && kbeg + CK < kend) load_chunk(kbeg + CK, pregs[PF - 1], wregs[PF - 1]);
    if (g.probe) tprobe[1] = wall_clock64();
    for (int cbase = kbeg; cbase < kend; cbase += PF * CK) {
#pragma unroll
        for (int s = 0; s < PF; ++s) {
            const int c0 = cbase + s * CK;
            if (c0 >= kend) break;
            __syncthreads();  // every wave is done reading the previous chunk
            if constexpr (NLOAD) {
                if (c0 < p.C0) {   // (uniform) a chunk of src0: this thread's 8 channels are the same in all of its items
                    const float* q = cst + c0 + (tid & 3) * EPS;
                    float nm[8], na[8], nb[8];
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const float4 m4 = *reinterpret_cast<const float4*>(q + 4 * h), a4 = *reinterpret_cast<const float4*>(q + C0r + 4 * h),
                                     b4 = *reinterpret_cast<const float4*>(q + 2 * C0r + 4 * h);
                        nm[4 * h] = m4.x; nm[4 * h + 1] = m4.y; nm[4 * h + 2] = m4.z; nm[4 * h + 3] = m4.w;
                        na[4 * h] = a4.x; na[4 * h + 1] = a4.y; na[4 * h + 2] = a4.z; na[4 * h + 3] = a4.w;
                        nb[4 * h] = b4.x; nb[4 * h + 1] = b4.y; nb[4 * h + 2] = b4.z; nb[4 * h + 3] = b4.w;
                    }
                    const bool segok = (tid & 3) * EPS < p.C0 - c0;
#pragma unroll
                    for (int i = 0; i < PITEMS; ++i) pregs[s][i] = nl_apply8(pregs[s][i], segok && poff0[i] >= 0, nm, na, nb);
                    if (p.nl_y && ytile == (c0 / CK) % g.ctiles) {     // (uniform) the activation tensor as a by-product, the chunks dealt round-robin to the
                                                                       // cout tiles of this pixel tile; out-of-range offsets are dropped by the hardware
                        const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(
                            (void*)((T*)p.nl_y + (size_t)n * H0 * W0 * p.C0), 0, H0 * W0 * p.C0 * (int)sizeof(T), 0x00020000);
#pragma unroll
                        for (int i = 0; i < PITEMS; ++i) {
                            const uint4 v = pregs[s][i];
                            __builtin_amdgcn_raw_buffer_store_b128(u32x4{v.x, v.y, v.z, v.w}, ry, (segok && ((ystore >> i) & 1u)) ? poff0[i] : (int)0x80000000,
                                                                   c0 * (int)sizeof(T), 0);
                        }
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < PITEMS; ++i) *reinterpret_cast<uint4*>(patch + pdst[i]) = pregs[s][i];
#pragma unroll
            for (int i = 0; i < WITEMS; ++i) {
                const bool full = (i + 1) * TS <= NTAPS;   // every row of this pass is a real tap
                const int dst = (full || wtap0 + i * TS < NTAPS) ? P * kPS + wdst0 + i * WROWS * kPS : dummy;
                *reinterpret_cast<uint4*>(smem + dst) = wregs[s][i];
            }
            __syncthreads();
            if (g.probe && c0 == kbeg) tprobe[2] = wall_clock64();
            if (c0 + PF * CK < kend) load_chunk(c0 + PF * CK, pregs[s], wregs[s]);  // in flight while the MFMAs of PF chunks run
            // fragments of tap t+1 are read while the MFMAs of tap t run (two register sets)
            uint4 wf[2][NJ], xf[2][PT];
            auto read_frags = [&](int tap, uint4 (&w)[NJ], uint4 (&x)[PT]) {
                const int kh = tap / KW, kw = tap % KW;
#pragma unroll
                for (int j = 0; j < NJ; ++j) w[j] = *reinterpret_cast<const uint4*>(wl + (tap * BN + j * 16) * kPS + wbase_l);
#pragma unroll
                for (int i = 0; i < PT; ++i) x[i] = *reinterpret_cast<const uint4*>(patch + xb[i][kw] + kh * khs);
            };
            constexpr int kMfmaPerTap = NJ * PT * (sizeof(T) == 2 ? 1 : 4);
            read_frags(0, wf[0], xf[0]);
            constexpr bool kPin = BN <= 32;   // 64-wide tiles run out of registers under the pinned order (measured slower)
            if (kPin) __builtin_amdgcn_sched_group_barrier(0x100, NJ + PT, 0);
#pragma unroll
            for (int tap = 0; tap < NTAPS; ++tap) {
                if (tap + 1 < NTAPS) read_frags(tap + 1, wf[(tap + 1) & 1], xf[(tap + 1) & 1]);
#pragma unroll
                for (int i = 0; i < PT; ++i)
#pragma unroll
                    for (int j = 0; j < NJ; ++j) mma16<T>(acc[i][j], wf[tap & 1][j], xf[tap & 1][i]);
                // pin the software pipeline: the LDS reads of tap t+1 issue before the MFMAs of tap t (left alone, the
                // scheduler serialises read -> wait -> MFMA to save registers)
                if (kPin && tap + 1 < NTAPS) __builtin_amdgcn_sched_group_barrier(0x100, NJ + PT, 0);
                if (kPin) __builtin_amdgcn_sched_group_barrier(0x008, kMfmaPerTap, 0);
            }
        }
    }

    if (g.probe) tprobe[3] = wall_clock64();
    conv_epilogue<T, BN, PT, NW>(p, tw_shift, g.out_nchw, n, h0, w0, n0, grp, acc, smem);
    if (g.probe) {
        __builtin_amdgcn_s_waitcnt(0);  // stores issued and acknowledged
        tprobe[4] = wall_clock64();
        if (tid == 0) {
            unsigned long long* o = g.probe + (size_t)blockIdx.x * 8;
            for (int i = 0; i < 5; ++i) o[i] = tprobe[i];
            unsigned hw, xcc;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
            o[5] = hw; o[6] = xcc; o[7] = 0;
        }
    }
}

// what the strip kernels (conv_strip.h: conv_direct_kernel, conv_head_kernel) cover
static bool direct_ok(int dtype, const ConvParams& p) {   // p.out_f32: bit 0 = fp32 store, bit 1 = NCHW layout
    const int CK = dtype == VS_F32 ? 16 : 32;
    const bool nchw = (p.out_f32 >> 1) != 0, f32 = (p.out_f32 & 1) != 0;
    const bool head_ok = p.Cout <= 4 && !p.pool0 && !p.scale && !p.relu && !p.up0 && !p.stats_partial;   // conv_head_kernel
    const bool out_ok = p.scatter ? (head_ok && (p.scatter->mode == 0 || (p.scatter->mode == 1 && p.scatter->keys)))
                                  : nchw ? (f32 && head_ok) : (!f32 && !(p.Cout & 3));
    return vs_option("conv_direct") && out_ok && !p.nl_bins && !p.bz && !p.gc && p.dil <= 1 && p.up0 != 2 && p.KH == 3 && p.KW == 3 && p.stride == 1 && p.pad == 1 && p.C1 == 0 && p.C0 <= CK &&
           p.Cout <= 16 && !p.residual && !p.out1 && (!p.pool0 || (!(p.Hout & 1) && !(p.Wout & 1) && p.Cout % 4 == 0)) &&
           (long)p.N * p.Hout * p.Wout >= (long)vs_option("conv_direct_min_px") &&
           (double)p.Hout * p.Wout * std::max(p.Cout, 4) * 4.0 < 2.0e9;
}

template <typename T, int BN, int PT, int NTAPS, int STRIDE, int NW = 4, int DIL = 1, bool NLOAD = false>
int launch_one(const ConvParams& p, const TileGeom& g, hipStream_t s) {
    static bool attr_set = false;
    auto kern = conv_igemm_kernel<T, BN, PT, NTAPS, STRIDE, NW, DIL, NLOAD>;
    const size_t lds = (size_t)g.PH * g.PW * kPS + (size_t)NTAPS * BN * kPS + 64 + (NLOAD ? (size_t)3 * ((p.C0 + 31) & ~31) * sizeof(float) : 0);
    VS_REQUIRE((double)p.Hin * p.Win * std::max(p.C0, p.C1) * sizeof(T) < 2.0e9 && (double)p.Cout * NTAPS * (p.C0 + p.C1) * sizeof(T) < 2.0e9,
               "conv_igemm: image or weight tensor exceeds the 32-bit staging offsets");
    VS_REQUIRE(lds <= 160 * 1024, "conv_igemm: LDS request %zu too large", lds);
    VS_REQUIRE(g.PH * g.PW * 4 <= patch_items(PT, DIL > 1 ? 2 : STRIDE, NW) * NW * 64, "conv_igemm: patch %dx%d exceeds the staging budget", g.PH, g.PW);
    if (!attr_set) {
        VS_CHECK_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        attr_set = true;
    }
    VS_REQUIRE(g.tiles_h * g.tiles_w < 65536 && p.N < 65536 && g.PH * g.PW + NW * 64 < 65536, "conv_igemm: tile grid too large");
    TileGeom gg = g;
    gg.groups = p.N * g.tiles_h * g.tiles_w;
    gg.ctiles = cdiv(p.Cout, BN);
    gg.ct_magic = 0xffffffffu / (unsigned)gg.ctiles + 1u;
    gg.ti_magic = 0xffffffffu / (unsigned)(g.tiles_h * g.tiles_w) + 1u;
    const long nwg = (long)cdiv(gg.groups, 8) * 8 * gg.ctiles;
    VS_REQUIRE(nwg < (1L << 31) && (long)gg.groups * (g.tiles_h * g.tiles_w) < (1L << 32), "conv_igemm: tile grid too large");
    if (g.probe) gg.probe = vs_probe_buffer((size_t)nwg);
    hipLaunchKernelGGL(kern, dim3((unsigned)nwg), dim3(NW * 64), lds, s, p, gg);
    VS_LAUNCH_CHECK();
    return VS_OK;
}

struct Pick { int BN, PT, NW; };
// tile width: static per kernel for stride 1 (see conv_igemm_kernel), by output width for stride 2
static int tile_tw(const ConvParams& p, int PT) { return p.stride == 1 ? (PT == 1 ? 8 : 16) : (p.Wout >= 16 ? 16 : 8); }

// One place decides the kernel configuration (cout tile, pixel tiles per wave, waves per workgroup):
//  * 8 waves x 2 pixel tiles = 256-pixel tiles for stride-1 layers with >= 16x16 outputs: half the weight-slab traffic per
//    FLOP of the 128-pixel tile, twice the waves per CU for latency hiding, half the staging registers per thread;
//  * 4 waves x 2 (128 px; also the stride-2 3x3 layers of large launches: 8x16 outputs) or x 1 (64 px: 8x8 images, stride 2)
//    otherwise;
//  * 32-wide cout tiles when 64-wide ones would leave fewer than `conv_min_wgs` workgroups.
Pick pick_cfg(const ConvParams& p) {
    Pick c;
    c.NW = 4;
    c.PT = (p.stride == 1 && p.Hout * p.Wout >= 128 && p.Wout >= 16) ? 2 : 1;
    if (p.stride == 2 && p.KH == 3 && p.Cout >= 64 && !p.gc && p.Wout >= 16 && p.Hout >= 8 &&
        (long)p.N * cdiv(p.Hout, 8) * cdiv(p.Wout, 16) * cdiv(p.Cout, 64) >= vs_option("conv_min_wgs")) c.PT = 2;
    const bool can8 = vs_option("conv_nw8") && p.stride == 1 && p.dil <= 1 && p.Hout >= 16 && p.Wout >= 16;
    auto wgs = [&](int bn, int px) {
        const int tw = tile_tw(p, px == 64 ? 1 : 2), th = px / tw;
        return (long)p.N * cdiv(p.Hout, th) * cdiv(p.Wout, tw) * cdiv(p.Cout, bn);
    };
    int bn = p.Cout >= 64 ? 64 : (p.Cout >= 32 ? 32 : 16);
    if (p.gc) bn = 32;     // grouped: one 32-channel super-group per cout tile
    if (p.out1 && p.split_c % 64 != 0 && bn == 64) bn = 32;   // a split data gradient (decoder concat): no cout tile may straddle the boundary (32 + 40
                                                               // channels under U-Net++ / efficientnet-b3)
    if (p.out1 && p.split_c % 32 != 0 && bn == 32) bn = 16;
    if (can8 && wgs(bn, 256) >= vs_option("conv_nw8_min_wgs")) { c.NW = 8; c.PT = 2; }
    if (bn == 64 && wgs(64, c.NW * c.PT * 16) < vs_option("conv_min_wgs")) bn = 32;
    c.BN = bn;
    return c;
}

// conv_ring_kernel (conv_ring.h) takes the deep stride-1 3x3 layers of small launches: >= 4 chunks of input channels
// (the ring needs a main loop to pay for its longer prologue) and grids of at most a few workgroups per CU, where one
// workgroup per CU with its staging off the registers beats two that stage through them (tools/convlab: layer2 / layer3 /
// layer4 / dec0 / dec1 shapes of the batch-32 step 12 - 22 % faster, the short-K 64- and 32-channel layers slower).
// 0 = no; 1 = 256-pixel tiles x 64 couts; 2 = 256-pixel tiles x 32 couts; 3 = pairs of 8 x 8 images x 32 couts
// conv_stream_kernel (conv_stream.h), the persistent form, takes the evaluation-mode stride-1 3x3 layers of LARGE launches
// (prediction: batches of 512 x 512 slices) - at least `conv_stream_min_tiles` tile jobs per CU-resident workgroup, so that
// the per-tile latencies it removes are what the launch consists of.  0 = no, else the cout tile (64 / 32)
static int stream_mode(int dtype, const ConvParams& p, int out_nchw) {
    if ((dtype != VS_BF16 && dtype != VS_F16) || !vs_option("conv_stream") || !ring::stream_ok(p, out_nchw) || p.C0 + p.C1 > 512 || p.nl_bins) return 0;
    const int bn = (p.Cout % 64 == 0) ? 64 : 32;
    const long jobs = (long)p.N * cdiv(p.Hout, 16) * cdiv(p.Wout, 16) * (p.Cout / bn);
    return jobs >= 256L * vs_option("conv_stream_min_tiles") ? bn : 0;
}

static int ring_mode(int dtype, const ConvParams& p, int out_nchw) {
    if (dtype != VS_BF16 || !vs_option("conv_ring") || p.KH != 3 || p.KW != 3 || p.stride != 1 || p.pad != 1 || p.dil > 1 || p.gc || p.scatter ||
        out_nchw || (p.Cout & 3) || p.out_f32) return 0;
    if (p.nl_bins && ((p.C0 & 31) || p.up0 == 2 || p.C0 > 1024)) return 0;   // normalise-on-load: whole chunks of src0, room for the table
    const int Cin = p.C0 + p.C1;
    if (Cin < 128 || (Cin & 7) || (p.C1 && (p.C0 & 31))) return 0;
    if (p.out1 && (p.split_c & 31)) return 0;
    if ((double)p.Hin * p.Win * std::max(p.C0, p.C1) * 2.0 * 2 >= 4.0e9) return 0;
    if (p.Hout == 8 && p.Wout == 8 && p.up0 == 0) {
        if (p.N % 2 == 0 && !p.pool0 && p.Cout >= 32 && (long)(p.N / 2) * cdiv(p.Cout, 32) <= 1024) return 3;
        return 0;
    }
    if (p.Hout < 16 || p.Wout < 16) return 0;
    const long tiles = (long)p.N * cdiv(p.Hout, 16) * cdiv(p.Wout, 16);
    const long w64 = tiles * cdiv(p.Cout, 64), w32 = tiles * cdiv(p.Cout, 32);
    const long maxw = vs_option("conv_ring_max_wgs");
    if (p.Cout >= 64 && w64 >= 224 && w64 <= maxw && (!p.out1 || p.split_c % 64 == 0)) return 1;
    if (p.Cout >= 32 && w32 >= 128 && w32 <= maxw) return 2;
    return 0;
}

// The tile family's instantiations, looked up from the full tuple: a tuple that is not listed has no kernel (it never runs a neighbour's).
constexpr int tile_key(int BN, int PT, int NW, int taps, int stride, int dil, bool nload) {
    return (((((BN * 4 + PT) * 16 + NW) * 16 + taps) * 4 + stride) * 8 + dil) * 2 + (nload ? 1 : 0);
}
template <typename T>
int launch_tile(const ConvParams& p, const ConvPlan& plan, const TileGeom& g, hipStream_t s) {
    constexpr bool kBf16 = std::is_same<T, bf16_t>::value;      // normalise-on-load is built for bf16 alone
#define VS_TILE(bn, pt, nw, taps, stride, dil, nload)                                                        \
    case tile_key(bn, pt, nw, taps, stride, dil, nload):                                                     \
        if constexpr (!nload || kBf16) return launch_one<T, bn, pt, taps, stride, nw, dil, nload>(p, g, s);  \
        break;
#define VS_TILE_32UP(...) VS_TILE(64, __VA_ARGS__) VS_TILE(32, __VA_ARGS__)
#define VS_TILE_BN(...) VS_TILE_32UP(__VA_ARGS__) VS_TILE(16, __VA_ARGS__)
    switch (tile_key(plan.BN, plan.PT, plan.NW, p.KH * p.KW, p.stride, p.dil > 1 ? p.dil : 1, p.nl_bins != nullptr)) {
        //      PT NW taps stride dil nload
        VS_TILE_BN(2, 4, 9, 1, 1, false) VS_TILE_BN(2, 4, 1, 1, 1, false)       // 128-pixel tiles
        VS_TILE_BN(1, 4, 9, 1, 1, false) VS_TILE_BN(1, 4, 1, 1, 1, false)       // 64-pixel tiles
        VS_TILE_BN(2, 8, 9, 1, 1, false) VS_TILE_BN(2, 8, 1, 1, 1, false)       // 8 waves: 256-pixel tiles
        VS_TILE_BN(1, 4, 9, 2, 1, false) VS_TILE_BN(1, 4, 1, 2, 1, false)       // stride 2
        VS_TILE(64, 2, 4, 9, 2, 1, false)                                       // 8 x 16 output tiles of the stride-2 3x3 layers of a big batch
        VS_TILE_32UP(2, 4, 9, 1, 2, false) VS_TILE_32UP(1, 4, 9, 1, 2, false)   // dilation 2: cout tiles of 32 and 64 only
        VS_TILE_32UP(2, 4, 9, 1, 4, false) VS_TILE_32UP(1, 4, 9, 1, 4, false)   // dilation 4
        VS_TILE_BN(2, 4, 9, 1, 1, true) VS_TILE_BN(1, 4, 9, 1, 1, true) VS_TILE_BN(2, 8, 9, 1, 1, true)   // normalise-on-load
    }
#undef VS_TILE_BN
#undef VS_TILE_32UP
#undef VS_TILE
    vs_set_error("conv_igemm: no kernel for BN=%d PT=%d NW=%d", plan.BN, plan.PT, plan.NW);
    return VS_ERR_UNSUPPORTED;
}

template <typename T>
int dispatch(const ConvParams& p, const ConvPlan& plan, hipStream_t s) {
    constexpr int CK = CT<T>::CK, EPS = CT<T>::EPS;
    const int Cin = p.C0 + p.C1, out_nchw = p.out_f32 >> 1;
    VS_REQUIRE(Cin % EPS == 0 && p.C0 % EPS == 0, "conv_igemm: channel counts must be multiples of %d", EPS);
    VS_REQUIRE(p.C1 == 0 || p.C0 % CK == 0, "conv_igemm: concat boundary must be a multiple of %d", CK);
    VS_REQUIRE(p.up0 >= 0 && p.up0 <= 2, "conv_igemm: up0 must be 0, 1 or 2");
    VS_REQUIRE(p.up0 != 2 || (p.C1 == 0 && !(p.Hin & 1) && !(p.Win & 1)), "conv_igemm: a zero-stuffed source has no concat partner and even dims");
    VS_REQUIRE(((p.KH == 3 && p.KW == 3) || (p.KH == 1 && p.KW == 1)) && (p.stride == 1 || p.stride == 2),
               "conv_igemm: unsupported kernel %dx%d stride %d", p.KH, p.KW, p.stride);
    const int dil = p.dil > 1 ? p.dil : 1;
    VS_REQUIRE(dil == 1 || ((dil == 2 || dil == 4) && p.KH == 3 && p.stride == 1 && p.Cout >= 32 && !p.pool0),
               "conv_igemm: dilation 2 / 4 is built for stride-1 3x3 layers of >= 32 channels");
    VS_REQUIRE(p.Hout == (p.Hin + 2 * p.pad - (p.KH - 1) * dil - 1) / p.stride + 1 && p.Wout == (p.Win + 2 * p.pad - (p.KW - 1) * dil - 1) / p.stride + 1,
               "conv_igemm: inconsistent output dims");
    VS_REQUIRE(p.src0 && p.w && (p.out || p.scatter), "conv_igemm: null pointer");
    VS_REQUIRE(p.gc == 0 || (p.gc == 32 && p.C1 == 0 && p.C0 == p.Cout && p.Cout % 32 == 0 && !p.out1),
               "conv_igemm: grouped convolutions run on 32-channel super-groups with as many inputs as outputs");
    VS_REQUIRE(!(out_nchw || (p.Cout & 3)) || (!p.out1), "conv_igemm: ragged / NCHW output cannot be split");
    const int BN = plan.BN, PT = plan.PT, NW = plan.NW;
    if (p.out1) VS_REQUIRE(p.split_c % BN == 0, "conv_igemm: split_c %d not a multiple of the cout tile %d", p.split_c, BN);
    if (p.bz) {
        VS_REQUIRE(!p.pool0 && !p.out1 && !p.scale && !p.shift && !p.relu && !p.out_f32 && !(p.Cout & 3) && !p.stats_partial &&
                   p.bmean && p.binvstd && p.bstats_partial && (!p.brelu || p.by || (p.bgamma && p.bbeta)),
                   "conv_igemm: the BN-backward epilogue takes a plain NHWC dgrad output");
    }
    if (p.pool0) {
        VS_REQUIRE(plan.can_pool && !p.residual && !p.scale && !p.shift && !out_nchw,
                   "conv_igemm: pooled dgrad epilogue not available for this geometry");
        VS_REQUIRE((p.out1 ? p.split_c : p.Cout) % 4 == 0, "conv_igemm: pooled channel count must be a multiple of 4");
    }
    if (p.nl_bins) {
        VS_REQUIRE(conv_igemm_nl_ok(Elem<T>::kDtype, p) && p.nl_mean && p.nl_invstd && p.nl_gamma && p.nl_beta && p.nl_nb >= 1 && p.nl_rows >= 1,
                   "conv_igemm: normalise-on-load is built for the bf16 stride-1 3x3 layers (ask conv_igemm_nl_ok first)");
    }
    ConvParams k = p;      // the point of launch: the kernels receive the fp32 bit alone, the layout bit travels in their geometry
    k.out_f32 = p.out_f32 & 1;
    if (plan.family == CONV_DIRECT) return strip::launch_direct<T>(k, out_nchw, s);
    if constexpr (sizeof(T) == 2) {
        if (plan.family == CONV_STREAM) {
            unsigned long long* probe = vs_probe_buffer(256);
            const int stg = 0;      // (a start delay staggered by workgroup was measured neutral)
            return BN == 64 ? ring::launch_stream<T, 64, 2, 8, 4, 2, 2>(k, probe, s, 256, stg) : ring::launch_stream<T, 32, 2, 8, 4, 2, 2>(k, probe, s, 256, stg);
        }
    }
    if constexpr (std::is_same<T, bf16_t>::value) {
        if (plan.family == CONV_RING) {
            const int rm = plan.ring;
            const long groups = rm == 3 ? p.N / 2 : (long)p.N * cdiv(p.Hout, 16) * cdiv(p.Wout, 16);
            unsigned long long* probe = vs_probe_buffer((size_t)(cdiv((int)groups, 8) * 8) * cdiv(p.Cout, BN));
            if (p.nl_bins) {
                if (rm == 1) return ring::launch_ring<64, 2, 8, 4, 1, 2, 2, true>(k, out_nchw, probe, s);
                if (rm == 2) return ring::launch_ring<32, 2, 8, 4, 1, 4, 2, true>(k, out_nchw, probe, s);
                return ring::launch_ring<32, 2, 4, 3, 2, 1, 2, true>(k, out_nchw, probe, s);
            }
            if (rm == 1) return ring::launch_ring<64, 2, 8, 4, 1, 2, 2>(k, out_nchw, probe, s);
            if (rm == 2) return ring::launch_ring<32, 2, 8, 4, 1, 4, 2>(k, out_nchw, probe, s);
            return ring::launch_ring<32, 2, 4, 3, 2, 1, 2>(k, out_nchw, probe, s);
        }
    }
    VS_REQUIRE(plan.family == CONV_TILE, "conv_igemm: the plan's kernel family %d is not built for this dtype", (int)plan.family);
    VS_REQUIRE(!p.scatter, "conv_igemm: the volume-scatter epilogue needs the direct kernel (check conv_head_scatter_ok first)");
    TileGeom g;
    g.tw_shift = tile_tw(p, PT) == 16 ? 4 : 3;
    const int TW = 1 << g.tw_shift;
    g.TH = NW * 16 * PT / TW;
    g.tiles_h = cdiv(p.Hout, g.TH);
    g.tiles_w = cdiv(p.Wout, TW);
    g.PH = (g.TH - 1) * p.stride + (p.KH - 1) * dil + 1;
    g.PW = (TW - 1) * p.stride + (p.KW - 1) * dil + 1;
    g.out_nchw = out_nchw;
    g.pw_magic = 0xffffffffu / (unsigned)g.PW + 1u;       // exact for x * PW < 2^32
    g.tw_magic = 0xffffffffu / (unsigned)g.tiles_w + 1u;
    g.probe = vs_probe_buffer((size_t)p.N * g.tiles_h * g.tiles_w * cdiv(p.Cout, BN));
    return launch_tile<T>(k, plan, g, s);
}

}  // namespace

// The one place that decides which kernel a launch gets: the families in their order of priority.  p as callers hold it
// (out_f32 packed); launch_conv_igemm and every query read what this returns.
ConvPlan conv_plan(int dtype, const ConvParams& p) {
    const int out_nchw = p.out_f32 >> 1, taps = p.KH * p.KW;
    const Pick c = pick_cfg(p);
    ConvPlan pl{};
    pl.can_pool = c.PT >= 2 && p.Wout >= 16 && !(p.Hout & 1) && !(p.Wout & 1);   // (the ring kernel's 16 x 16 tiles: the same condition)
    if (direct_ok(dtype, p)) {   // (a 32-cout form was measured in round 4: 636 vs 426 us for the tile kernel on the 32 -> 32 layer of a 128 x 512^2 batch - not kept)
        pl.family = CONV_DIRECT; pl.BN = 16; pl.PT = 2; pl.NW = 4;
        pl.stat_rows = strip::direct_geom(p).nwaves;   // one partial row per wave
        pl.code = 16 * 1000 + 2 * 100 + 9 * 10 + 4;
        return pl;
    }
    const int sm = stream_mode(dtype, p, out_nchw), rm = ring_mode(dtype, p, out_nchw);
    const int TW = tile_tw(p, c.PT), TH = c.NW * 16 * c.PT / TW;
    pl.stat_rows = rm ? (rm == 3 ? p.N / 2 : p.N * cdiv(p.Hout, 16) * cdiv(p.Wout, 16)) : p.N * cdiv(p.Hout, TH) * cdiv(p.Wout, TW);
    if (sm) {
        pl.family = CONV_STREAM; pl.BN = sm; pl.PT = 2; pl.NW = 8;
        pl.code = sm * 1000 + 2 * 100 + 9 * 10 + 7;
    } else if (rm) {
        pl.family = CONV_RING; pl.ring = rm; pl.BN = rm == 1 ? 64 : 32; pl.PT = 2; pl.NW = rm == 3 ? 4 : 8;
        pl.code = pl.BN * 1000 + 2 * 100 + 9 * 10 + 6;
    } else {
        pl.family = CONV_TILE; pl.BN = c.BN; pl.PT = c.PT; pl.NW = c.NW;
        pl.code = c.BN * 1000 + c.PT * 100 + taps * 10 + (c.NW == 8 ? 8 : (p.stride == 2 ? 2 : 1));
    }
    return pl;
}

bool head_dgrad_planes_ok(int dtype, int classes, int H, int W, int C) {
    return (dtype == VS_BF16 || dtype == VS_F16) && classes >= 1 && 9 * classes <= 64 && C >= 4 && C <= 16 && !(C & 3) &&
           (double)classes * H * W < 2.0e9 && (double)H * W * C * 2.0 < 2.0e9;
}
int launch_head_dgrad_planes(int dtype, const float* dl, const void* w, void* out, int N, int classes, int H, int W, int C, hipStream_t s) {
    VS_REQUIRE(head_dgrad_planes_ok(dtype, classes, H, W, C), "head_dgrad_planes: unsupported shape (classes %d, %d x %d x %d)", classes, H, W, C);
    return strip::launch_head_dgrad(dtype, dl, w, out, N, classes, H, W, C, s);
}

// whether launch_conv_igemm can normalise p.src0 while loading it (ConvParams::nl_*): the register-staged tile kernel's bf16
// stride-1 3x3 instantiations (p as the layer will be launched, nl_* set or not)
bool conv_igemm_nl_ok(int dtype, const ConvParams& p) {
    ConvParams q = p;
    q.nl_bins = nullptr;
    if (dtype != VS_BF16 || p.KH != 3 || p.KW != 3 || p.stride != 1 || p.pad != 1 || p.dil > 1 || p.gc || p.scatter || p.up0 == 2 || p.bz ||
        (p.C0 & 7) || p.C0 > 2048) return false;
    return conv_plan(dtype, q).family != CONV_DIRECT;    // the strip kernels have no such loader (yet)
}

int launch_conv_igemm(int dtype, const ConvParams& p, hipStream_t s, const ConvPlan* plan) {
    const ConvPlan pl = plan ? *plan : conv_plan(dtype, p);
    if (dtype == VS_BF16) return dispatch<bf16_t>(p, pl, s);
    if (dtype == VS_F32) return dispatch<float>(p, pl, s);
    if (dtype == VS_F16) {
        VS_REQUIRE(!p.bz && !p.stats_partial && !p.pool0, "conv_igemm: fp16 is the inference precision (no training epilogues)");
        return dispatch<f16_t>(p, pl, s);
    }
    vs_set_error("conv_igemm: bad dtype %d", dtype);
    return VS_ERR_INVALID;
}

// Whether two chained evaluation-mode layers - p's output (NHWC, storage type) read by q and by nothing else - can run as ONE launch of
// conv_direct_pair_kernel: both are strip-kernel layers on their own (CONV_DIRECT), 16-bit storage, at most 16 channels between them.
bool conv_pair_ok(int dtype, const ConvParams& p, const ConvParams& q) {
    if ((dtype != VS_BF16 && dtype != VS_F16) || !vs_option("conv_pair")) return false;
    if (conv_plan(dtype, p).family != CONV_DIRECT || conv_plan(dtype, q).family != CONV_DIRECT) return false;
    if (p.pool0 || q.pool0 || p.scatter || q.scatter || p.out_f32 || q.out_f32 || p.stats_partial || p.stats_bins || q.stats_partial || q.stats_bins ||
        q.up0 || q.C1 || p.Cout > 16 || q.Cout > 16 || (p.Cout & 7) || (q.Cout & 3)) return false;
    return q.C0 == p.Cout && q.N == p.N && q.Hin == p.Hout && q.Win == p.Wout && q.Hout == p.Hout && q.Wout == p.Wout;
}

int launch_conv_pair(int dtype, const ConvParams& p, const ConvParams& q, hipStream_t s) {
    VS_REQUIRE(conv_pair_ok(dtype, p, q), "conv_pair: the two layers cannot share a launch (ask conv_pair_ok first)");
    VS_REQUIRE(p.src0 && p.w && q.w && q.out, "conv_pair: null pointer");
    VS_REQUIRE((double)p.Hin * p.Win * p.C0 * 2.0 < 2.0e9 && (double)q.Hout * q.Wout * q.Cout * 2.0 < 2.0e9, "conv_pair: tensor too large");
    return strip::launch_pair(dtype, p, q, s);
}
