// The passes over a network plan (unet_plan.h): everything that enqueues.
//
// A plan is a flat list of units with all activation, gradient and scratch buffers laid out once in a caller-owned workspace;
// unet_plan.hip builds it for every supported topology and encoder, and this file moves none of it.  vs_unet_forward / vs_unet_backward
// enqueue every kernel of a step from C++ on the caller's stream - Python makes one call per pass.  Forward in training mode keeps
// the pre-norm (z) and post-activation (a) tensors; backward walks the units in reverse with a statically known first-write /
// accumulate discipline for the gradients of tensors with several consumers (ResNet identities, skips), and runs the weight gradients
// and the fused optimiser step on side streams.  In file order: the side streams, the launch context and descriptors, the optimiser
// step of a range of units, the units (one forward and one backward function per kind), the weight-gradient share of a backward call,
// the two loops, the C entry points.
#include <cstdlib>
#include <cmath>
#include <string>
#include <vector>

#include "common.h"
#include "prof.h"
#include "unet_plan.h"

using namespace unet;

// ---- the side streams: one pair per device for every plan of the process, checked against the caller's stream -------------------
// HIP multiplexes its streams onto a few hardware queues (GPU_MAX_HW_QUEUES, 4 by default).  A side stream that shares its queue with
// the caller's stream runs its kernels IN ORDER with the caller's: the weight gradients no longer overlap the backward pass and the
// batch-32 step takes 5.3 instead of 4.4 ms - measured for every second model a process creates when each plan made its own streams
// (tools/placement_probe.py, profiles/r4_side_stream_hw_queues.txt).  So the streams are made once, and the first time they serve a
// given caller's stream a 2 x 100 us timing probe (one spin kernel on each stream, started together) tells whether the two really run
// beside one another; a stream that does not is parked (kept, so that the runtime's assignment moves on) and another one is tried.
__global__ void side_probe_spin(unsigned long long ticks) {   // ticks of the 100 MHz wall clock
    const unsigned long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
}
struct SidePool {
    hipStream_t s[vs_unet::kSide] = {nullptr, nullptr};
    hipStream_t checked_for = nullptr;
    bool checked = false;
    std::vector<hipStream_t> parked;
};
static SidePool& side_pool() {
    static SidePool pools[64];
    int dev = 0;
    (void)hipGetDevice(&dev);
    return pools[dev & 63];
}
// true: a kernel on `a` and a kernel on `b` ran at the same time
static int streams_overlap(hipStream_t a, hipStream_t b, bool* yes) {
    hipEvent_t e0, e1, eb;
    VS_CHECK_HIP(hipEventCreate(&e0));
    VS_CHECK_HIP(hipEventCreate(&e1));
    VS_CHECK_HIP(hipEventCreateWithFlags(&eb, hipEventDisableTiming));
    VS_CHECK_HIP(hipStreamSynchronize(a));
    VS_CHECK_HIP(hipStreamSynchronize(b));
    float best = 1e30f;
    for (int rep = 0; rep < 2; ++rep) {       // (the first pass also pays the kernel's load)
        VS_CHECK_HIP(hipEventRecord(e0, a));
        hipLaunchKernelGGL(side_probe_spin, dim3(1), dim3(64), 0, a, 10000ull);
        hipLaunchKernelGGL(side_probe_spin, dim3(1), dim3(64), 0, b, 10000ull);
        VS_CHECK_HIP(hipEventRecord(eb, b));
        VS_CHECK_HIP(hipStreamWaitEvent(a, eb, 0));
        VS_CHECK_HIP(hipEventRecord(e1, a));
        VS_CHECK_HIP(hipStreamSynchronize(a));
        float ms = 0.f;
        VS_CHECK_HIP(hipEventElapsedTime(&ms, e0, e1));
        best = std::min(best, ms);
    }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipEventDestroy(eb);
    *yes = best < 0.160f;                     // two 100 us kernels: ~0.11 ms beside one another, ~0.21 ms one after the other
    return VS_OK;
}
static int acquire_side_streams(vs_unet* net, hipStream_t caller) {
    SidePool& pool = side_pool();
    for (int i = 0; i < vs_unet::kSide; ++i)
        if (!pool.s[i]) VS_CHECK_HIP(hipStreamCreateWithFlags(&pool.s[i], hipStreamNonBlocking));
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(caller, &cap);
    if (cap == hipStreamCaptureStatusNone && !(pool.checked && pool.checked_for == caller)) {
        for (int i = 0; i < vs_unet::kSide; ++i) {
            for (int attempt = 0; attempt < 8; ++attempt) {
                bool ok = false;
                const int rc = streams_overlap(caller, pool.s[i], &ok);
                if (rc) return rc;
                if (ok && i == 1) { const int rc2 = streams_overlap(pool.s[0], pool.s[1], &ok); if (rc2) return rc2; }
                if (ok) break;
                pool.parked.push_back(pool.s[i]);
                VS_CHECK_HIP(hipStreamCreateWithFlags(&pool.s[i], hipStreamNonBlocking));
            }
        }
        pool.checked = true;
        pool.checked_for = caller;
    }
    for (int i = 0; i < vs_unet::kSide; ++i) net->side[i] = pool.s[i];
    return VS_OK;
}

namespace {

// ---- the launch context of a pass and the launch descriptors of a unit ------------------------------------------------------------
struct Ctx {
    vs_unet* net;
    char* ws;
    const float* params;
    float* bnstate;
    hipStream_t s;
    int n;
    void* a(int id) const { return ws + net->acts[id].off_a; }
    void* z(int id) const { return ws + net->acts[id].off_z; }
    void* da(int id) const { return ws + net->acts[id].off_da; }
    void* dz(int id) const { return ws + net->acts[id].off_dz; }
    const TensorInfo& t(int idx) const { return net->layout.tensors[idx]; }
    const float* P(int idx) const { return params + t(idx).offset; }
    const void* wfwd(const Unit& u) const {  // weights in the compute dtype
        return has_weight_copy(net, u) ? (const void*)(ws + wc_off(u, net->wset)) : (const void*)P(u.w_idx);
    }
    static size_t wc_off(const Unit& u, int set) { return set ? u.off_wc2 : u.off_wc; }
    static size_t wt_off(const Unit& u, int set) { return set ? u.off_wt2 : u.off_wt; }
    float* bnc(const Unit& u, int which) const { return reinterpret_cast<float*>(ws + u.off_bn) + (size_t)which * u.cout; }
    int64_t rows(const Unit& u) const { return (int64_t)n * u.hout * u.wout; }
    float* rmean(const Unit& u) const { return u.bn_idx >= 0 ? bnstate + t(u.bn_idx + 2).offset : nullptr; }   // running statistics (forward)
    float* rvar(const Unit& u) const { return u.bn_idx >= 0 ? bnstate + t(u.bn_idx + 3).offset : nullptr; }
    float* bnws() const { return reinterpret_cast<float*>(ws + net->off_bnws); }    // the BatchNorm / column-sum partial rows
    // the weight gradients' split-K slab buffer number `slab` (one per stream that runs them), and the dense 3x3 gradient next to it
    float* wgws(int slab) const { return reinterpret_cast<float*>(ws + net->off_wgws + (size_t)slab * net->wgws_bytes); }
    float* ctdw(int slab) const { return reinterpret_cast<float*>(ws + net->off_ctdw + (size_t)slab * net->ctdw_bytes); }
    // do `rows` partial rows of 2 * cout floats fit that workspace
    bool bnws_fits(int rows, int cout) const { return (size_t)rows * 2 * cout * sizeof(float) <= net->bnws_bytes; }
};

// THE weight-copy row of a convolution unit (U_CONV / U_HEAD) in weight set `set`: where its copies go and the shape the copy kernel
// sees - a large-rate convolution (colr) is the 1x1 convolution over the 9 * cin0 channels of the column form, the head's transposed
// copy pads to 16 output channels, cg = 255 marks the two-group layout.  wc only where the forward reads a copy (has_weight_copy);
// want_wt: the flipped / transposed copy of the data gradient; update: the fused optimiser step runs AdamW on the weight.
WeightCopyRow weight_copy_row(const vs_unet* net, const Unit& u, int set, bool want_wt, bool update) {
    WeightCopyRow r;
    r.w_off = net->layout.tensors[u.w_idx].offset;
    r.wc_off = has_weight_copy(net, u) ? (long)Ctx::wc_off(u, set) : -1;
    r.wt_off = want_wt ? (long)Ctx::wt_off(u, set) : -1;
    r.cout = u.cout; r.taps = u.colr ? 1 : u.k * u.k; r.cin = u.colr ? 9 * u.cin0 : u.cin0 + u.cin1;
    r.cout_pad = u.kind == U_HEAD ? 16 : u.cout;
    r.cg = u.g2 ? 255 : u.cg;
    r.update = update;
    return r;
}

double conv_flops(const Ctx& c, const Unit& u) {  // algorithmic: 2 * MACs of the (un-padded, un-stuffed) convolution
    return 2.0 * c.n * u.hout * u.wout * (double)u.cout * u.k * u.k * (u.cg ? u.cg : u.cin0 + u.cin1);
}
double act_bytes(const Ctx& c, const Unit& u, int passes) {  // `passes` full sweeps over the unit's output tensor
    return (double)passes * c.n * u.hout * u.wout * u.cout * c.net->esz;
}

ConvParams conv_params(const Ctx& c, const Unit& u) {
    ConvParams p{};
    p.src0 = c.a(u.src0);
    p.src1 = u.src1 >= 0 ? c.a(u.src1) : nullptr;
    p.C0 = u.cin0; p.C1 = u.cin1; p.up0 = u.up0;
    p.N = c.n; p.Hin = u.hin; p.Win = u.win; p.Hout = u.hout; p.Wout = u.wout;
    p.stride = u.stride; p.pad = u.pad; p.KH = p.KW = u.k;
    p.w = c.wfwd(u); p.Cout = u.cout;
    p.gc = u.cg ? 32 : 0;
    p.dil = u.dil;
    if (u.colr) { p.src0 = c.ws + u.off_xs; p.C0 = 9 * u.cin0; p.pad = 0; p.KH = p.KW = 1; }   // the 1x1 form over the column form
    if (u.kind == U_CONVT) {   // its 3x3 form: same-size output, 4 * cout channels, always from the prepared copy
        p.Hout = u.hin; p.Wout = u.win; p.Cout = 4 * u.cout;
        p.w = c.ws + Ctx::wc_off(u, c.net->wset);
    }
    return p;
}

// the weight-gradient launch of a convolution unit, without dy / dw / workspace
WgradParams wgrad_params(const Ctx& c, const Unit& u) {
    WgradParams p{};
    p.src0 = c.a(u.src0); p.src1 = u.src1 >= 0 ? c.a(u.src1) : nullptr;
    p.C0 = u.cin0; p.C1 = u.cin1; p.up0 = u.up0; p.N = c.n; p.Hin = u.hin; p.Win = u.win;
    p.Hout = u.hout; p.Wout = u.wout; p.stride = u.stride; p.pad = u.pad; p.KH = p.KW = u.k;
    p.Cout = u.cout;
    p.cg = u.cg; p.dil = u.dil;
    if (u.colr) { p.src0 = c.ws + u.off_xs; p.C0 = 9 * u.cin0; p.pad = 0; p.KH = p.KW = 1; }
    return p;
}

// Normalise-on-load (training, bf16): unit ui is a conv -> BN -> ReLU whose output has exactly ONE reader, a stride-1 3x3
// convolution that takes it as src0 (a BasicBlock's conv1 -> conv2; a decoder block's conv1 -> conv2 -> next block's conv1).
// Then ui runs no normalisation sweep: its statistics stay in their fixed-point bins, the reader's workgroups sum them in their
// prologue, normalise ui's PRE-norm tensor while staging it and leave the normalised activation behind as a by-product for the
// weight gradient (ConvParams::nl_*).  THE answer to "does unit ui leave its output un-normalised for its reader at batch c.n", every
// precondition included (the forward and vs_unet_nl_plan both ask here): the reader's unit index, or -1.
int nl_consumer(const Ctx& c, int ui) {
    vs_unet* net = c.net;
    const int dt = net->dtype;
    const Unit& u = net->units[ui];
    if (dt != VS_BF16 || !vs_option("nl_fwd") || net->stats_hook) return -1;   // (cross-rank statistics: the sweep finalises)
    if (!vs_option("stats_bins") || !net->bins_bytes) return -1;              // (the reader finalises the producer's bins)
    if (u.kind != U_CONV || u.relu != 1 || u.res >= 0 || u.colr || u.gn_idx >= 0 || u.bias_idx >= 0 || u.bn_idx < 0 || u.cout > 512 ||
        u.cout > vs_option("nl_max_c")) return -1;    // (the reader's table and per-chunk work grow with the channel count: per-unit table in DESIGN.md)
    ensure_graph_maps(net);
    const int vi = net->sole_consumer[u.out];
    if (vi <= ui) return -1;
    const Unit& v = net->units[vi];
    if (v.kind != U_CONV || v.src0 != u.out || v.src1 == u.out || v.res == u.out || v.colr || v.cg || v.g2) return -1;
    if (!conv_igemm_nl_ok(dt, conv_params(c, v))) return -1;
    return vi;
}

// AdamW over the parameter slices of the units [lo, hi) (everything, minus the frozen encoder convolutions when those are
// not trained) and the derived weight copies of their convolutions for the NEXT forward (the other weight set), on `s`.
int update_units(const Ctx& c, int lo, int hi, bool need_encoder_wgrad, const float* grads, const vs_adamw_args& opt,
                 hipStream_t s) {
    vs_unet* net = c.net;
    const int dt = net->dtype;
    const int other = net->wset ^ 1;
    AdamwRanges r{};
    WeightCopyRow rows[64];
    int nl = 0;
    int rc;
    // Per range of units: ONE launch steps the small tensors (BatchNorm affine parameters, biases, the stem, depthwise / attention
    // tensors: ranges of the flat buffers), ONE launch steps the convolution weights INSIDE the derivation of their copies for the next
    // forward (round 4: the AdamW launch over the group's convolution slices and the copy launch were two; 0.025 ms per step)
    auto flush = [&]() -> int {
        int rc2;
        if (r.n && (rc2 = launch_adamw_ranges(opt, grads, r, s))) return rc2;
        if (nl && (rc2 = launch_adamw_prepare_all(dt, opt, grads, c.ws, rows, nl, s))) return rc2;
        r.n = 0; nl = 0;
        return VS_OK;
    };
    auto push = [&](int idx) {
        const TensorInfo& t = c.t(idx);
        const int64_t len = tensor_elems(t);
        if (r.n > 0 && r.off[r.n - 1] + r.len[r.n - 1] == t.offset) { r.len[r.n - 1] += len; return; }
        r.off[r.n] = t.offset; r.len[r.n] = len; ++r.n;
    };
    for (int k = lo; k < hi; ++k) {
        const Unit& v = net->units[k];
        if (v.w_idx < 0 && v.bn_idx < 0) continue;
        if (r.n > 150 || nl == 64) { if ((rc = flush())) return rc; }
        if (v.kind == U_SE) { push(v.w_idx); push(v.w_idx + 1); push(v.w_idx + 2); push(v.w_idx + 3); continue; }
        if (v.kind == U_FPA) { for (int t : v.tens) push(t); continue; }
        const bool conv_w = v.kind == U_CONV || v.kind == U_HEAD;          // its weight is updated by the fused copy launch below
        if (v.w_idx >= 0 && !conv_w && !(v.frozen_candidate && !need_encoder_wgrad)) push(v.w_idx);
        const bool aux_on = !(v.aux_frozen && !need_encoder_wgrad);      // (ResNeSt: BatchNorms / biases named conv2.bn0, conv2.fc1, conv1.1 ..)
        if (v.bn_idx >= 0 && aux_on) { push(v.bn_idx); push(v.bn_idx + 1); }
        if (v.gn_idx >= 0) { push(v.gn_idx); push(v.gn_idx + 1); }
        if (v.bias_idx >= 0 && aux_on) push(v.bias_idx);
        if (conv_w) rows[nl++] = weight_copy_row(net, v, other, true, !(v.frozen_candidate && !need_encoder_wgrad));
    }
    if ((rc = flush())) return rc;
    for (int k = lo; k < hi; ++k) {   // transposed convolutions: their own expansion kernel, after every AdamW launch of the range
        const Unit& v = net->units[k];
        if (v.kind != U_CONVT) continue;
        if ((rc = launch_convt_weight_prepare(dt, opt.params + c.t(v.w_idx).offset, c.ws + Ctx::wc_off(v, other), c.ws + Ctx::wt_off(v, other),
                                              v.cin0, v.cout, s))) return rc;
    }
    return VS_OK;
}

// ---- the units ---------------------------------------------------------------------------------------
// Per kind: what it computes, the function that enqueues its forward and, right behind it, its backward.  The kinds with a weight of
// their own (stem, convolutions, head) have a backward in three parts, because the pass puts a fork event between the first two and
// runs the third on another stream: the norm half (_bwd_norm: the output's gradient -> dz, the gradient w.r.t. the convolution's
// output, + the norm's / bias' own gradients), the data gradient (_bwd_data: dz -> the inputs' gradients) and the weight gradient
// (_wgrad).  unet_forward / unet_backward_range below only walk the units and dispatch.
#define VS_TRY(expr) do { if (const int rc_ = (expr)) return rc_; } while (0)

// Arguments and loop-carried state of one forward pass
struct Fwd {
    const float* x; float* logits; int training; const VolScatter* scatter;
    int ui = -1;                   // the unit being enqueued: set by the loop, read by the units that look at the unit behind them
    int skip_units = 0;            // units that already ran inside this unit's launch: set by U_CONV (evaluation: conv_pair, the U_BN behind it)
                                   // and U_DWCONV2 (evaluation: the U_BN behind it), consumed by the loop
    int carried_stat_rows = 0;     // partial statistic rows a plain U_CONV's epilogue left in bnws (training): consumed by the U_BN right behind it
    bool head_scattered = false;   // set by U_HEAD: its kernel wrote the volume entries itself; read by unet_forward's return value
};
// Where train_norm finds the batch statistics of the unit it normalises: the per-unit state of the forward, set by the unit's
// convolution and handed over as an argument.  NONE: no sweep follows (the one reader normalises on load).
struct Stats { enum Source { NONE, SWEEP, BINS, ROWS } source; int rows; };   // rows: partial rows in bnws (ROWS)

// The gradient-written protocol of a backward pass, over vs_unet::written (kept in the plan: a pass may come as several ranges).  A
// kind states per input whether it overwrites (first) or may find earlier contributions (next); nothing else touches written[].
struct Ledger {
    std::vector<char>& written;
    int ui = -1, kind = -1;        // the unit at work, for the messages: set by the loop
    int need(int act) const {      // the gradient of `act` must be present
        VS_REQUIRE(written[act], "backward: unit %d (kind %d) reads the gradient of activation %d, which nothing has written", ui, kind, act);
        return VS_OK;
    }
    int first(int act) {           // first and only writer of the gradient of `act`
        VS_REQUIRE(!written[act], "backward: unit %d (kind %d) overwrites the gradient of activation %d, which is already written", ui, kind, act);
        written[act] = 1;
        return VS_OK;
    }
    int next(int act) {            // one more writer: 1 = accumulate onto what is there, 0 = this is the first
        const int acc = written[act] ? 1 : 0;
        written[act] = 1;
        return acc;
    }
};
// Arguments of one backward call and its ledger
struct Bwd {
    const float* x; const float* dlogits; float* grads; bool need_encoder_wgrad; const vs_adamw_args* opt;
    Ledger g;
    float* grad(const Ctx& c, int tensor) const { return grads + c.t(tensor).offset; }
    bool want_w(const Unit& u) const { return !(u.frozen_candidate && !need_encoder_wgrad); }   // else: the weight's gradient is zeroed
};

// Where the dz of a weighted unit lives once its norm half has run, and its channel count: THE lookup of both roles
struct Dz { const void* p; int c; };
Dz unit_dz(const Ctx& c, const Unit& u) {
    if (u.kind == U_HEAD) return {c.ws + c.net->off_dyh, 16};               // dlogits as 16-channel NHWC
    if (u.kind == U_CONVT) return {c.da(u.out), 4 * u.cout};                // of the 3x3 form, in the unit's (by then dead) da buffer
    const bool no_norm = u.kind == U_DWCONV || u.kind == U_DWCONV2 || (u.kind == U_CONV && u.bn_idx < 0 && u.gn_idx < 0);
    return {no_norm ? c.da(u.out) : c.dz(u.out), u.cout};                   // no norm, no activation: dz IS the output's gradient
}

// Training: batch statistics + normalise (+ residual) (+ ReLU) of the pre-norm tensor z of a unit with its own BatchNorm
int train_norm(const Ctx& c, const Unit& u, Stats st) {
    vs_unet* net = c.net;
    const int dt = net->dtype;
    if (st.source == Stats::NONE) return VS_OK;   // normalise-on-load: no sweep, no activation tensor
    float *rm = c.rmean(u), *rv = c.rvar(u);
    const void* res = u.res >= 0 ? c.a(u.res) : nullptr;
    if (st.source == Stats::BINS) {
        int64_t stat_rows = 0;
        if (net->stats_hook) {     // SyncBatchNorm: the integer sums of every rank, added in place (exact: the same bits everywhere)
            const int hrc = net->stats_hook(net->stats_user, c.ws + u.off_bins, (int64_t)stat_bins_rows(u.cout) * 2 * u.cout, 0, (void*)c.s);
            VS_REQUIRE(hrc == 0, "unet_forward: the cross-rank statistics hook failed (%d)", hrc);
            stat_rows = c.rows(u) * net->stats_world;
        }
        ProfScope prof(PK_BN_APPLY, 0, act_bytes(c, u, u.res >= 0 ? 3 : 2), c.s);
        return launch_bn_apply_from_bins(dt, c.z(u.out), (const unsigned long long*)(c.ws + u.off_bins), stat_bins_rows(u.cout), 1e-5f, 0.1f,
                                         c.bnc(u, 2), c.bnc(u, 3), rm, rv, c.P(u.bn_idx), c.P(u.bn_idx + 1), res, u.relu, c.a(u.out), c.rows(u), u.cout,
                                         c.s, stat_rows);
    }
    VS_REQUIRE(!net->stats_hook, "unet_forward: cross-rank BatchNorm statistics need the statistics bins for every unit (bf16, options stats_bins / fuse_stats)");
    if (st.source == Stats::ROWS && st.rows <= vs_option("bn_inline_rows")) {   // few partial rows: one launch does both
        ProfScope prof(PK_BN_APPLY, 0, act_bytes(c, u, u.res >= 0 ? 3 : 2), c.s);
        return launch_bn_apply_from_partials(dt, c.z(u.out), c.bnws(), st.rows, 1e-5f, 0.1f, c.bnc(u, 2), c.bnc(u, 3), rm, rv, c.P(u.bn_idx),
                                             c.P(u.bn_idx + 1), res, u.relu, c.a(u.out), c.rows(u), u.cout, c.s);
    }
    if (st.source == Stats::ROWS) {
        ProfScope prof(PK_BN_STATS, 0, 0, c.s);
        VS_TRY(launch_bn_finalize_partials(c.bnws(), st.rows, u.cout, c.rows(u), 1e-5f, 0.1f, c.bnc(u, 2), c.bnc(u, 3), rm, rv, c.s));
    } else {
        ProfScope prof(PK_BN_STATS, 0, act_bytes(c, u, 1), c.s);
        VS_TRY(vs_bn_stats(dt, c.z(u.out), c.rows(u), u.cout, 1e-5f, 0.1f, c.bnc(u, 2), c.bnc(u, 3), rm, rv, c.bnws(), net->bnws_bytes, c.s));
    }
    ProfScope prof(PK_BN_APPLY, 0, act_bytes(c, u, u.res >= 0 ? 3 : 2), c.s);
    return vs_bn_apply(dt, c.z(u.out), c.bnc(u, 2), c.bnc(u, 3), c.P(u.bn_idx), c.P(u.bn_idx + 1), res, u.relu, c.a(u.out), c.rows(u), u.cout, c.s);
}

// Backward of that BatchNorm (+ ReLU, + residual): da(out) -> dz(out), the residual's gradient, dgamma, dbeta
int train_norm_bwd(const Ctx& c, const Unit& u, Bwd& b) {
    vs_unet* net = c.net;
    const int dt = net->dtype;
    VS_TRY(b.g.need(u.out));
    void* dres = nullptr;
    if (u.res >= 0) {
        VS_TRY(b.g.first(u.res));
        dres = c.da(u.res);
    }
    BnSync sy{net->stats_hook, net->stats_user, net->stats_world, (float*)(c.ws + net->off_syncsc)};
    const BnSync* sync = net->stats_hook ? &sy : nullptr;
    if (net->bwd_stat_rows[u.out] > 0) {
        // the dgrad that completed da(u.out) left the masked gradient and the reduction's partial rows: one sweep
        ProfScope prof(PK_BN_BWD, 0, act_bytes(c, u, 3 + (dres ? 1 : 0)), c.s);
        VS_TRY(launch_bn_bwd_from_partials(dt, c.da(u.out), c.z(u.out), c.bnc(u, 2), c.bnc(u, 3), c.P(u.bn_idx), c.dz(u.out), dres, b.grad(c, u.bn_idx),
                                           b.grad(c, u.bn_idx + 1), c.rows(u), u.cout, c.bnws(), net->bwd_stat_rows[u.out], c.s, sync));
        net->bwd_stat_rows[u.out] = 0;
        return VS_OK;
    }
    // two sweeps: (dy, y, x) reduce, then (dy, y, x) -> dx (+ dres)
    const bool recompute_mask = u.relu && u.res < 0;  // mask from x: two tensor reads fewer
    ProfScope prof(PK_BN_BWD, 0, act_bytes(c, u, ((u.relu && !recompute_mask) ? 6 : 4) + 1 + (dres ? 1 : 0)), c.s);
    return bn_bwd_dispatch(dt, c.da(u.out), recompute_mask ? nullptr : c.a(u.out), c.z(u.out), c.bnc(u, 2), c.bnc(u, 3), c.P(u.bn_idx),
                           c.P(u.bn_idx + 1), u.relu, c.dz(u.out), dres, b.grad(c, u.bn_idx), b.grad(c, u.bn_idx + 1), c.rows(u), u.cout, c.bnws(),
                           net->bnws_bytes, c.s, sync);
}

// The head's data gradient reads dLoss / dlogits straight from its planes where head_dgrad_planes_kernel applies; the 16-channel NHWC
// form (+ the bias gradient of the same sweep) is then only the weight gradient's operand and is made on ITS stream.
bool head_reads_planes(const Ctx& c, const Unit& u) {
    const vs_unet* net = c.net;
    return vs_option("conv_direct") != 0 &&    // (the strip-kernel family's switch)
           u.k == 3 && u.stride == 1 && u.pad == 1 && u.dil <= 1 && !u.cg && u.cin1 == 0 && !u.up0 &&
           net->first_consumer[u.src0] == (int)net->units.size() - 1 &&     // (the head, the plan's last unit, is its input's only reader)
           head_dgrad_planes_ok(net->dtype, net->classes, u.hout, u.wout, u.cin0);
}
// dLoss / dlogits at the head's own resolution (behind the backward of its bilinear upsampling, where it has one)
const float* head_dlogits(const Ctx& c, const Bwd& b) {
    return c.net->head_up > 1 ? (const float*)(c.ws + c.net->off_dlsmall) : b.dlogits;
}

// U_STEM: the ResNet stem, Conv2d(1, 64, 7, stride 2, padding 3) + BN + ReLU on the network input
int stem_fwd(const Ctx& c, const Unit& u, Fwd& f) {
    vs_unet* net = c.net;
    const int dt = net->dtype, n = c.n;
    Stats stats{Stats::SWEEP, 0};
    {
        ProfScope prof(PK_STEM, 2.0 * n * u.hout * u.wout * 64 * 49, 4.0 * n * net->h * net->w + act_bytes(c, u, 1), c.s);
        if (f.training && u.cout == 64 && net->bins_bytes && vs_option("stats_bins") && stem_fwd_bins_ok(dt)) {
            // batch statistics from the kernel's own accumulators (fixed-point bins, finalised inside the apply sweep)
            VS_TRY(launch_stem_fwd_bins(f.x, c.P(u.w_idx), c.z(u.out), n, net->h, net->w, (unsigned long long*)(c.ws + u.off_bins),
                                        stat_bins_rows(u.cout), c.s));
            stats.source = Stats::BINS;
        } else if (f.training && net->stats_hook) {
            vs_set_error("unet_forward: cross-rank BatchNorm statistics need the bf16 stem kernel and the statistics bins (options stem_bf16, stats_bins, fuse_stats)");
            return VS_ERR_UNSUPPORTED;
        } else if (f.training) {
            VS_TRY(vs_stem_fwd(dt, f.x, c.P(u.w_idx), nullptr, nullptr, 0, c.z(u.out), n, net->h, net->w, c.s));
        } else {
            VS_TRY(vs_stem_fwd(dt, f.x, c.P(u.w_idx), c.bnc(u, 0), c.bnc(u, 1), 1, c.a(u.out), n, net->h, net->w, c.s));
        }
    }
    return f.training ? train_norm(c, u, stats) : VS_OK;
}
int stem_bwd_norm(const Ctx& c, const Unit& u, Bwd& b) { return train_norm_bwd(c, u, b); }
// (no data gradient: its input is the network's)
int stem_wgrad(const Ctx& c, const Unit& u, const Bwd& b, Dz dz, hipStream_t s, int slab) {
    const vs_unet* net = c.net;
    const bool want_w = b.want_w(u);
    ProfScope prof(PK_STEM, want_w ? 2.0 * c.n * u.hout * u.wout * 64 * 49 : 0, 0, s);
    if (want_w) return vs_stem_wgrad(net->dtype, b.x, dz.p, b.grad(c, u.w_idx), c.wgws(slab), net->wgws_bytes, c.n, net->h, net->w, (void*)s);
    VS_CHECK_HIP(hipMemsetAsync(b.grad(c, u.w_idx), 0, tensor_elems(c.t(u.w_idx)) * sizeof(float), s));
    return VS_OK;
}

// U_POOL: nn.MaxPool2d(3, 2, 1) behind the stem; training keeps the arg-max indices
int pool_fwd(const Ctx& c, const Unit& u, Fwd& f) {
    const vs_unet* net = c.net;
    ProfScope prof(PK_POOL_MISC, 0, (double)c.n * u.hin * u.win * 64 * net->esz * 1.25, c.s);
    return vs_maxpool_fwd(net->dtype, c.a(u.src0), c.a(u.out), f.training ? (uint8_t*)(c.ws + net->off_idx) : nullptr, c.n, u.hin, u.win, u.cout, c.s);
}
int pool_bwd(const Ctx& c, const Unit& u, Bwd& b) {
    const vs_unet* net = c.net;
    VS_TRY(b.g.need(u.out));
    ProfScope prof(PK_POOL_MISC, 0, (double)c.n * u.hin * u.win * 64 * net->esz * 1.5, c.s);
    return vs_maxpool_bwd(net->dtype, c.da(u.out), (const uint8_t*)(c.ws + net->off_idx), c.da(u.src0), b.g.next(u.src0), c.n, u.hin, u.win, u.cout, c.s);
}

// U_CONV: a convolution (dense, grouped cg, two-group g2, dilated dil, large-rate colr; on cat(up(src0), src1) where up0 / src1 say so)
// followed by BatchNorm (+ residual) (+ ReLU), by GroupNorm + ReLU (gn_idx), or by nothing but its bias (bn_idx < 0: FPN's lateral
// 1x1s, EfficientNet's 1x1s whose norm is the U_BN behind them)
int conv_fwd_launch(const Ctx& c, const Unit& u, Fwd& f, Stats& stats) {
    vs_unet* net = c.net;
    const int dt = net->dtype, n = c.n;
    ConvParams p = conv_params(c, u);
    if (f.training && u.src0 >= 0 && net->nl_act[u.src0]) {   // src0 ran no normalisation sweep: its pre-norm tensor, normalised while it is staged
        const Unit& q = net->units[net->producer[u.src0]];
        p.src0 = c.z(u.src0);
        p.nl_bins = (const unsigned long long*)(c.ws + q.off_bins); p.nl_nb = stat_bins_rows(q.cout);
        p.nl_rows = c.rows(q); p.nl_eps = 1e-5f; p.nl_mom = 0.1f;
        p.nl_mean = c.bnc(q, 2); p.nl_invstd = c.bnc(q, 3);
        p.nl_rm = c.rmean(q); p.nl_rv = c.rvar(q);
        p.nl_gamma = c.P(q.bn_idx); p.nl_beta = c.P(q.bn_idx + 1);
        p.nl_y = c.a(u.src0);      // the activation the weight gradient reads: this launch's by-product
    }
    const ConvPlan plan = conv_plan(dt, p);     // (before the epilogue fields are set: a launch behind one of those decides again)
    prof_set_variant(plan.code);
    ProfScope prof(PK_CONV_FWD, conv_flops(c, u), 0, c.s);
    prof_set_variant(0);
    if (u.bn_idx < 0 && u.gn_idx < 0) {   // plain biased convolution: no norm, no activation
        p.out = c.a(u.out); p.shift = u.bias_idx >= 0 ? c.P(u.bias_idx) : nullptr;   // (EfficientNet's 1x1 convolutions: no bias either)
        // its BatchNorm is the next unit (U_BN): the batch statistics come straight from the fp32 accumulators, as for the fused units
        const Unit* next_bn = bn_behind(net, f.ui);
        if (f.training && dt == VS_BF16 && u.bias_idx < 0 && next_bn && plan.stat_rows > 0 && c.bnws_fits(plan.stat_rows, u.cout)) {
            p.stats_partial = c.bnws();
            f.carried_stat_rows = plan.stat_rows;
        }
        // evaluation: the BatchNorm unit behind it (folded running statistics) and its activation ride in this epilogue
        if (!f.training && u.bias_idx < 0 && next_bn) {
            const Unit& bn = *next_bn;
            p.scale = c.bnc(bn, 0); p.shift = c.bnc(bn, 1); p.relu = bn.relu; p.out = c.a(bn.out);
            f.skip_units = 1;
        }
        return launch_conv_igemm(dt, p, c.s);
    }
    if (u.colr) VS_TRY(vs_dilated_im2col(dt, c.a(u.src0), c.ws + u.off_xs, n, u.hin, u.win, u.cin0, u.colr, 0, 0, c.s));
    if (u.gn_idx >= 0) {                  // convolution + GroupNorm + ReLU (per-sample statistics: nothing folds in evaluation)
        p.out = f.training ? c.z(u.out) : (void*)(c.ws + net->off_gnz);
        VS_TRY(launch_conv_igemm(dt, p, c.s, &plan));
        return vs_gn_fwd(dt, p.out, c.P(u.gn_idx), c.P(u.gn_idx + 1), u.relu, c.a(u.out), (float*)(c.ws + u.off_gn), n, (int64_t)u.hout * u.wout, u.cout,
                         u.gn_groups, 1e-5f, (float*)(c.ws + net->off_gnws), net->gnws_bytes, c.s);
    }
    if (f.training) {
        stats = {Stats::SWEEP, 0};
        p.out = c.z(u.out);
        if (u.bias_idx >= 0) p.shift = c.P(u.bias_idx);   // smp's ConvBnRelu keeps the convolution's bias: z includes it
        if (dt == VS_BF16 && u.bias_idx < 0) {  // batch statistics straight from the fp32 accumulators
            const int rows_needed = plan.stat_rows;
            const bool bins_ok = u.bn_idx >= 0 && vs_option("stats_bins") && net->bins_bytes;   // (every bf16 kernel has them)
            const bool nl = nl_consumer(c, f.ui) >= 0;
            if (nl || (bins_ok && (net->stats_hook || rows_needed > vs_option("bn_inline_rows")))) {
                // many tiles: their sums go into a few rows of fixed-point bins, finalised inside the apply sweep -
                // no finalize launch between the convolution and its normalisation (0.34 ms of a 4.76 ms step)
                p.stats_bins = (unsigned long long*)(c.ws + u.off_bins);
                p.stats_nb = stat_bins_rows(u.cout);
                stats = {nl ? Stats::NONE : Stats::BINS, 0};
                if (nl) net->nl_act[u.out] = 1;   // no sweep: the one reader finalises the bins and normalises on load
            } else if (c.bnws_fits(rows_needed, u.cout)) {
                p.stats_partial = c.bnws();
                if (rows_needed) stats = {Stats::ROWS, rows_needed};
            }
        }
    } else {
        p.out = c.a(u.out);
        p.scale = c.bnc(u, 0); p.shift = c.bnc(u, 1);
        p.residual = u.res >= 0 ? c.a(u.res) : nullptr;
        p.relu = u.relu;
        // evaluation: this layer and the next one - its only reader, a plain conv + BN + ReLU - as ONE launch when both are
        // strip-kernel layers (smp's last decoder block at full resolution): the tensor between them is never written
        ensure_graph_maps(net);
        const int vi = f.ui + 1;
        if (vi < (int)net->units.size() && net->sole_consumer[u.out] == vi && u.res < 0 && u.bias_idx < 0 && u.bn_idx >= 0) {
            const Unit& v = net->units[vi];
            if (v.kind == U_CONV && v.src0 == u.out && v.src1 < 0 && !v.up0 && v.res < 0 && v.bn_idx >= 0 && v.gn_idx < 0 && v.bias_idx < 0 &&
                !v.colr && !v.cg && !v.g2) {
                ConvParams q = conv_params(c, v);
                q.out = c.a(v.out); q.scale = c.bnc(v, 0); q.shift = c.bnc(v, 1); q.relu = v.relu;
                ConvParams p1 = p;
                p1.out = nullptr;
                p1.out_f32 = 0; q.out_f32 = 0;
                if (conv_pair_ok(dt, p1, q)) {
                    VS_TRY(launch_conv_pair(dt, p1, q, c.s));
                    prof_add_flops(conv_flops(c, v));
                    f.skip_units = 1;
                    return VS_OK;
                }
            }
        }
    }
    return launch_conv_igemm(dt, p, c.s);
}
int conv_fwd(const Ctx& c, const Unit& u, Fwd& f) {
    Stats stats{Stats::NONE, 0};      // stays so in evaluation and where no BatchNorm of the unit's own follows
    VS_TRY(conv_fwd_launch(c, u, f, stats));
    return train_norm(c, u, stats);
}
int conv_bwd_norm(const Ctx& c, const Unit& u, Bwd& b) {
    const vs_unet* net = c.net;
    const int dt = net->dtype, n = c.n;
    if (u.bn_idx < 0 && u.gn_idx < 0) {   // plain biased convolution: the bias gradient = column sums of the output's gradient
        VS_TRY(b.g.need(u.out));
        ProfScope prof(PK_POOL_MISC, 0, (double)n * u.hout * u.wout * u.cout * net->esz, c.s);
        if (u.bias_idx >= 0) VS_TRY(vs_colsum(dt, c.da(u.out), c.rows(u), u.cout, b.grad(c, u.bias_idx), c.bnws(), net->bnws_bytes, c.s));
        return VS_OK;
    }
    if (u.gn_idx >= 0) {                  // GroupNorm + ReLU backward
        VS_TRY(b.g.need(u.out));
        ProfScope prof(PK_BN_BWD, 0, act_bytes(c, u, 5), c.s);
        return vs_gn_bwd(dt, c.da(u.out), c.z(u.out), (const float*)(c.ws + u.off_gn), c.P(u.gn_idx), c.P(u.gn_idx + 1), u.relu, c.dz(u.out),
                         b.grad(c, u.gn_idx), b.grad(c, u.gn_idx + 1), n, (int64_t)u.hout * u.wout, u.cout, u.gn_groups, (float*)(c.ws + net->off_gnws),
                         net->gnws_bytes, c.s);
    }
    VS_TRY(train_norm_bwd(c, u, b));
    if (u.bias_idx >= 0)    // a biased convolution in front of BatchNorm (smp's ConvBnRelu): column sums of dz
        VS_TRY(vs_colsum(dt, c.dz(u.out), c.rows(u), u.cout, b.grad(c, u.bias_idx), c.bnws(), net->bnws_bytes, c.s));
    return VS_OK;
}
// large-rate convolution: the data gradient of the 1x1 form = the input gradient's column form; its adjoint scatter onto the map
int conv_colr_bwd_data(const Ctx& c, const Unit& u, Bwd& b, Dz dz) {
    const vs_unet* net = c.net;
    const int dt = net->dtype, n = c.n;
    ConvParams p{};
    p.src0 = dz.p; p.C0 = u.cout; p.N = n; p.Hin = p.Hout = u.hin; p.Win = p.Wout = u.win; p.stride = 1; p.pad = 0; p.KH = p.KW = 1;
    p.w = c.ws + Ctx::wt_off(u, net->wset); p.Cout = 9 * u.cin0; p.out = c.ws + net->off_ys;
    {
        ProfScope prof(PK_CONV_DGRAD, conv_flops(c, u), 0, c.s);
        VS_TRY(launch_conv_igemm(dt, p, c.s));
    }
    return vs_dilated_im2col(dt, p.out, c.da(u.src0), n, u.hin, u.win, u.cin0, u.colr, 1, b.g.next(u.src0), c.s);
}
// The data gradient of a convolution unit (U_CONV, U_CONVT, U_HEAD without the planes kernel): the convolution of dz with the
// flipped / transposed weight copy
int conv_bwd_data(const Ctx& c, const Unit& u, Bwd& b, Dz dz) {
    vs_unet* net = c.net;
    const int dt = net->dtype, n = c.n, ui = b.g.ui;
    if (u.colr) return conv_colr_bwd_data(c, u, b, dz);
    ConvParams p{};
    const void* dsrc = dz.p;
    const bool stuff_in_loader = u.stride == 2 && !(u.hin & 1) && !(u.win & 1);
    if (u.stride == 2 && !stuff_in_loader) {
        void* zs = c.ws + net->off_zs;
        ProfScope prof(PK_POOL_MISC, 0, (double)n * u.hin * u.win * dz.c * net->esz * 1.25, c.s);
        VS_TRY(vs_zero_stuff2x(dt, dz.p, zs, n, u.hout, u.wout, dz.c, c.s));
        dsrc = zs;
    }
    p.src0 = dsrc; p.C0 = dz.c; p.N = n; p.Hin = u.hin; p.Win = u.win; p.Hout = u.hin; p.Wout = u.win;
    if (stuff_in_loader) p.up0 = 2;   // the patch loader reads dz at the even positions and zeros elsewhere
    p.stride = 1; p.pad = u.pad; p.KH = p.KW = u.k;
    p.w = c.ws + Ctx::wt_off(u, net->wset); p.Cout = u.cin0 + u.cin1;
    p.gc = u.cg ? 32 : 0;
    p.dil = u.dil;
    if (u.up0) {
        // U-Net: every decoder input has this one consumer.  U-Net++: the upsampled input may already hold the contributions
        // of the nodes that read it as a dense skip - then the 2x2 sum goes through the separate, accumulating kernel.
        const int acc0 = b.g.next(u.src0);
        if (u.src1 >= 0) {
            VS_TRY(b.g.first(u.src1));
            p.out1 = c.da(u.src1); p.split_c = u.cin0;
        }
        if (!acc0 && conv_plan(dt, p).can_pool) {  // 2x2 sum of the upsampled part inside the dgrad epilogue
            p.pool0 = 1;
            p.out = c.da(u.src0);
            const ConvPlan plan = conv_plan(dt, p);
            prof_set_variant(plan.code);
            ProfScope prof(PK_CONV_DGRAD, conv_flops(c, u), 0, c.s);
            prof_set_variant(0);
            return launch_conv_igemm(dt, p, c.s, &plan);
        }
        p.out = c.ws + net->off_dup;
        {
            ProfScope prof(PK_CONV_DGRAD, conv_flops(c, u), 0, c.s);
            VS_TRY(launch_conv_igemm(dt, p, c.s));
        }
        ProfScope prof(PK_POOL_MISC, 0, (double)n * u.hin * u.win * u.cin0 * net->esz * 1.25, c.s);
        return launch_upsample2x_bwd(dt, p.out, c.da(u.src0), n, u.hin / 2, u.win / 2, u.cin0, acc0, c.s);
    }
    p.out = c.da(u.src0);
    p.residual = b.g.next(u.src0) ? c.da(u.src0) : nullptr;
    // If this is the LAST contribution to the gradient of a conv+BN unit's activation and that unit is processed
    // next, its BN-backward reduction can ride in this epilogue (mask, masked store, per-tile partial sums).  Opt-in
    // (fuse_bn_bwd = 1): measured neutral per step.  Per layer (bench.py --per-unit) the BN sweep gets 5-14 us shorter and
    // the dgrad 3-17 us longer: the fused form saves ONE tensor read (the gradient itself) and a launch, but the
    // epilogue reads z / y / earlier contributions 8 bytes per lane (16 scattered 32-byte pieces per instruction) at
    // the tail of every workgroup, which costs about what the separate, fully coalesced sweep cost.  Layers the direct kernel takes
    // are left alone (it has no such epilogue; falling back to the tile kernel cost 55 us each).
    const int pa = u.src0, pu = net->producer[pa];
    ConvPlan plan = conv_plan(dt, p);
    if (vs_option("fuse_bn_bwd") && pu >= 0 && pu == ui - 1 && net->first_consumer[pa] == ui && net->units[pu].kind == U_CONV &&
        net->units[pu].bn_idx >= 0 && !(p.Cout & 3) && plan.family != CONV_DIRECT) {
        const Unit& q = net->units[pu];
        const int rows_needed = plan.stat_rows;
        // (fixed-point bins for these sums - no finalize launch - were measured in round 3: -0.013 ms per step, and they are not
        // scale-equivariant (gradients of 2 g != 2 x gradients of g bit for bit): not kept)
        if (c.bnws_fits(rows_needed, q.cout)) {
            const bool recompute = q.relu && q.res < 0;
            p.bz = c.z(q.out);
            p.by = (q.relu && !recompute) ? c.a(q.out) : nullptr;
            p.bmean = c.bnc(q, 2); p.binvstd = c.bnc(q, 3);
            p.bgamma = c.P(q.bn_idx); p.bbeta = c.P(q.bn_idx + 1);
            p.bstats_partial = c.bnws();
            p.brelu = q.relu;
            net->bwd_stat_rows[pa] = rows_needed;
            plan = conv_plan(dt, p);      // bz is set: the BN-backward epilogue narrows the choice
        }
    }
    prof_set_variant(plan.code);
    ProfScope prof(PK_CONV_DGRAD, u.kind == U_HEAD ? 2.0 * n * u.hout * u.wout * net->classes * u.k * u.k * u.cin0 : conv_flops(c, u), 0, c.s);
    prof_set_variant(0);
    return launch_conv_igemm(dt, p, c.s, &plan);
}
// The weight gradient of a convolution unit (U_CONV, U_CONVT, U_HEAD) on stream s, with slab buffer `slab`
int conv_wgrad(const Ctx& c, const Unit& u, const Bwd& b, Dz dz, hipStream_t s, int slab) {
    const vs_unet* net = c.net;
    const int dt = net->dtype, n = c.n;
    if (!b.want_w(u)) {
        VS_CHECK_HIP(hipMemsetAsync(b.grad(c, u.w_idx), 0, tensor_elems(c.t(u.w_idx)) * sizeof(float), s));
        return VS_OK;
    }
    ProfScope prof(PK_CONV_WGRAD, conv_flops(c, u), 0, s);
    WgradParams p = wgrad_params(c, u);
    p.dy = dz.p; p.Cout = dz.c;
    p.partials = c.wgws(slab); p.partial_bytes = net->wgws_bytes;
    if (u.kind == U_CONVT) {   // dense gradient of the 3x3 form, then its 16 real taps into torch's [in][out][4][4]
        p.Hout = u.hin; p.Wout = u.win;
        p.dw = c.ctdw(slab);
        VS_TRY(launch_conv_wgrad(dt, p, s));
        return launch_convt_wgrad_gather(p.dw, b.grad(c, u.w_idx), u.cin0, u.cout, s);
    }
    if (u.g2) {        // dense gradient, then every output channel's own group half into the [cout][taps][cin / 2] tensor
        p.dw = c.ctdw(slab);
        VS_TRY(launch_conv_wgrad(dt, p, s));
        return launch_two_group_wgrad_extract(p.dw, b.grad(c, u.w_idx), u.cout, u.k * u.k, u.cin0, s);
    }
    if (u.kind == U_HEAD) {
        p.cout_live = net->classes;
        if (head_reads_planes(c, u)) {    // the bias gradient, and - unless the weight-gradient kernel reads the planes itself - its 16-channel operand: off the caller's stream
            const float* head_dl = head_dlogits(c, b);
            p.dy_planes = net->classes;
            const bool direct = conv_wgrad_takes_planes(dt, p) && n <= 256;   // (the bias-only sweep's partial buffer: 4 segments x 256 images)
            if (direct) p.dy = head_dl; else p.dy_planes = 0;
            VS_TRY(launch_dlogits_to_nhwc16(dt, head_dl, direct ? nullptr : c.ws + net->off_dyh, n, net->classes, (int64_t)u.hout * u.wout,
                                            b.grad(c, u.bias_idx), (float*)(c.ws + net->off_headpart), s));
        }
        if (conv_wgrad_honours_cout_live(dt, p)) {   // the row-streaming kernel leaves [classes][9][16] slabs: summed straight into the gradient
            p.dw = b.grad(c, u.w_idx);
            return launch_conv_wgrad(dt, p, s);
        }
        p.cout_live = 0;
        p.dw = (float*)(c.ws + net->off_headdw);
        VS_TRY(launch_conv_wgrad(dt, p, s));
        VS_CHECK_HIP(hipMemcpyAsync(b.grad(c, u.w_idx), p.dw, tensor_elems(c.t(u.w_idx)) * sizeof(float), hipMemcpyDeviceToDevice, s));
        return VS_OK;
    }
    // (the split-K slabs are summed right behind the kernel, out of the ONE slab buffer every layer reuses: it stays in the
    // L2s / Infinity Cache.  Round 4 measured the alternatives: slabs kept per layer and summed once per optimiser group
    // (+0.02 ms per step: 0.7 GB of slabs then go to HBM and back) or inside the optimiser launch (+0.33 ms))
    p.dw = b.grad(c, u.w_idx);
    return launch_conv_wgrad(dt, p, s);
}

// U_HEAD: the segmentation head, Conv2d(c, classes, k) + bias -> fp32 NCHW logits (+ nn.UpsamplingBilinear2d(head_up)); in prediction
// its epilogue can write the volume entries itself (scatter)
int head_fwd(const Ctx& c, const Unit& u, Fwd& f) {
    const vs_unet* net = c.net;
    const int dt = net->dtype;
    ConvParams p = conv_params(c, u);
    p.out = f.logits; p.shift = c.P(u.bias_idx); p.out_f32 = 3;  // fp32, NCHW
    ProfScope prof(PK_HEAD, conv_flops(c, u), 0, c.s);
    if (net->head_up > 1) {   // SegmentationHead(upsampling=4): the convolution at 1/4 resolution, then nn.UpsamplingBilinear2d
        p.out = c.ws + net->off_lsmall;
        VS_TRY(launch_conv_igemm(dt, p, c.s));
        return vs_bilinear_up_planes((const float*)p.out, f.logits, c.n * net->classes, u.hout, u.wout, net->head_up, c.s);
    }
    if (f.scatter) {
        p.scatter = f.scatter;
        const ConvPlan plan = conv_plan(dt, p);
        if (conv_head_scatter_ok(p, plan)) {
            p.out = nullptr;
            VS_TRY(launch_conv_igemm(dt, p, c.s, &plan));
            f.head_scattered = true;
            return VS_OK;
        }
        p.scatter = nullptr;
    }
    return launch_conv_igemm(dt, p, c.s);
}
int head_bwd_norm(const Ctx& c, const Unit& u, Bwd& b) {
    const vs_unet* net = c.net;
    const int n = c.n;
    {
        ProfScope prof(PK_HEAD, 0, (double)n * net->h * net->w * (net->classes * 8 + 16 * net->esz), c.s);
        if (net->head_up > 1)     // back through the head's bilinear upsampling first
            VS_TRY(vs_bilinear_up_planes_bwd(b.dlogits, (float*)(c.ws + net->off_dlsmall), n * net->classes, u.hout, u.wout, net->head_up, c.s));
    }
    if (head_reads_planes(c, u)) return VS_OK;
    ProfScope prof(PK_HEAD, 0, (double)n * net->h * net->w * (net->classes * 8 + 16 * net->esz), c.s);
    return launch_dlogits_to_nhwc16(net->dtype, head_dlogits(c, b), c.ws + net->off_dyh, n, net->classes, (int64_t)u.hout * u.wout, b.grad(c, u.bias_idx),
                                    c.bnws(), c.s);   // + bias gradient, same sweep
}
int head_bwd_data(const Ctx& c, const Unit& u, Bwd& b, Dz dz) {
    const vs_unet* net = c.net;
    if (!head_reads_planes(c, u)) return conv_bwd_data(c, u, b, dz);
    VS_TRY(b.g.first(u.src0));
    ProfScope prof(PK_CONV_DGRAD, 2.0 * c.n * u.hout * u.wout * net->classes * u.k * u.k * u.cin0, 0, c.s);
    return launch_head_dgrad_planes(net->dtype, head_dlogits(c, b), c.ws + Ctx::wc_off(u, net->wset), c.da(u.src0), c.n, net->classes, u.hout, u.wout,
                                    u.cin0, c.s);
}

// U_CONCAT: torch.cat of U-Net++'s dense skips, materialised (one channel-slice copy per member); members = the activations whose
// channels `out` strings together, in order
int concat_fwd(const Ctx& c, const Unit& u, Fwd&) {
    const vs_unet* net = c.net;
    ProfScope prof(PK_POOL_MISC, 0, 2.0 * c.n * u.hout * u.wout * u.cout * net->esz, c.s);
    int off = 0;
    for (int m : u.members) {
        const int mc = net->acts[m].c;
        VS_TRY(vs_channel_slice(net->dtype, c.a(m), mc, 0, c.a(u.out), u.cout, off, mc, c.rows(u), 0, c.s));
        off += mc;
    }
    return VS_OK;
}
int concat_bwd(const Ctx& c, const Unit& u, Bwd& b) {   // each slice is added onto its member's gradient
    const vs_unet* net = c.net;
    VS_TRY(b.g.need(u.out));
    ProfScope prof(PK_POOL_MISC, 0, 3.0 * c.n * u.hout * u.wout * u.cout * net->esz, c.s);
    int off = 0;
    for (int m : u.members) {
        const int mc = net->acts[m].c;
        VS_TRY(vs_channel_slice(net->dtype, c.da(u.out), u.cout, off, c.da(m), mc, 0, mc, c.rows(u), b.g.next(m), c.s));
        off += mc;
    }
    return VS_OK;
}

// U_CONVT: ConvTranspose2d(4, stride 2, padding 1) + BN + ReLU (smp Linknet's TransposeX2): a 3x3 convolution onto 4 * cout channels
// (conv_igemm) + pixel shuffle (+ bias; evaluation: + folded BN + ReLU); cin0 -> cout channels, hin x win -> hout x wout = 2x
int convt_fwd(const Ctx& c, const Unit& u, Fwd& f) {
    const vs_unet* net = c.net;
    const int dt = net->dtype, n = c.n;
    ConvParams p = conv_params(c, u);
    p.out = c.ws + net->off_ct;
    {
        ProfScope prof(PK_CONV_FWD, conv_flops(c, u) * 4, 0, c.s);
        VS_TRY(launch_conv_igemm(dt, p, c.s));
    }
    {
        ProfScope prof(PK_POOL_MISC, 0, 2.0 * n * u.hout * u.wout * u.cout * net->esz, c.s);
        if (f.training) VS_TRY(vs_depth_to_space2(dt, p.out, c.z(u.out), n, u.hin, u.win, u.cout, c.P(u.bias_idx), nullptr, nullptr, 0, c.s));
        else VS_TRY(vs_depth_to_space2(dt, p.out, c.a(u.out), n, u.hin, u.win, u.cout, c.P(u.bias_idx), c.bnc(u, 0), c.bnc(u, 1), u.relu, c.s));
    }
    return f.training ? train_norm(c, u, Stats{Stats::SWEEP, 0}) : VS_OK;
}
int convt_bwd_norm(const Ctx& c, const Unit& u, Bwd& b) {
    const vs_unet* net = c.net;
    const int dt = net->dtype, n = c.n;
    VS_TRY(train_norm_bwd(c, u, b));
    // the bias gradient (column sums of dz), then dz back through the pixel shuffle: the gradient of the 3x3 form's
    // output, kept in the (now dead) da buffer of this unit - the side stream's weight gradient reads it later
    ProfScope prof(PK_POOL_MISC, 0, 3.0 * n * u.hout * u.wout * u.cout * net->esz, c.s);
    VS_TRY(vs_colsum(dt, c.dz(u.out), c.rows(u), u.cout, b.grad(c, u.bias_idx), c.bnws(), net->bnws_bytes, c.s));
    return vs_space_to_depth2(dt, c.dz(u.out), c.da(u.out), n, u.hin, u.win, u.cout, c.s);
}
// (data gradient and weight gradient: conv_bwd_data / conv_wgrad on the 3x3 form)

// U_ADD: out = a(src0) + a(src1) (Linknet's skip connection, FPN's merge)
int add_fwd(const Ctx& c, const Unit& u, Fwd&) {
    const int dt = c.net->dtype;
    ProfScope prof(PK_POOL_MISC, 0, 3.0 * c.n * u.hout * u.wout * u.cout * c.net->esz, c.s);
    VS_TRY(vs_channel_slice(dt, c.a(u.src0), u.cout, 0, c.a(u.out), u.cout, 0, u.cout, c.rows(u), 0, c.s));
    return vs_channel_slice(dt, c.a(u.src1), u.cout, 0, c.a(u.out), u.cout, 0, u.cout, c.rows(u), 1, c.s);
}
int add_bwd(const Ctx& c, const Unit& u, Bwd& b) {      // both addends receive the sum's gradient
    VS_TRY(b.g.need(u.out));
    ProfScope prof(PK_POOL_MISC, 0, 4.0 * c.n * u.hout * u.wout * u.cout * c.net->esz, c.s);
    for (int m : {u.src0, u.src1})
        VS_TRY(vs_channel_slice(c.net->dtype, c.da(u.out), u.cout, 0, c.da(m), u.cout, 0, u.cout, c.rows(u), b.g.next(m), c.s));
    return VS_OK;
}

// U_UPADD: out = nearest-x2 upsampling of a(src0) + a(src1) (smp FPNBlock)
int upadd_fwd(const Ctx& c, const Unit& u, Fwd&) {
    ProfScope prof(PK_POOL_MISC, 0, 2.25 * c.n * u.hout * u.wout * u.cout * c.net->esz, c.s);
    return vs_upsample2x_add(c.net->dtype, c.a(u.src0), c.a(u.src1), c.a(u.out), c.n, u.hin, u.win, u.cout, c.s);
}
int upadd_bwd(const Ctx& c, const Unit& u, Bwd& b) {    // the lateral addend takes the gradient as is, the upsampled one its 2x2 sums
    const int dt = c.net->dtype;
    VS_TRY(b.g.need(u.out));
    ProfScope prof(PK_POOL_MISC, 0, 3.5 * c.n * u.hout * u.wout * u.cout * c.net->esz, c.s);
    VS_TRY(vs_channel_slice(dt, c.da(u.out), u.cout, 0, c.da(u.src1), u.cout, 0, u.cout, c.rows(u), b.g.next(u.src1), c.s));
    return launch_upsample2x_bwd(dt, c.da(u.out), c.da(u.src0), c.n, u.hin, u.win, u.cout, b.g.next(u.src0), c.s);
}

// U_BILINEAR: out = bilinear x `factor` upsampling (align_corners) of a(src0) (smp Conv3x3GNReLU(upsample=True))
int bilinear_fwd(const Ctx& c, const Unit& u, Fwd&) {
    ProfScope prof(PK_POOL_MISC, 0, 1.25 * c.n * u.hout * u.wout * u.cout * c.net->esz, c.s);
    return vs_bilinear_up(c.net->dtype, c.a(u.src0), c.a(u.out), c.n, u.hin, u.win, u.cout, u.factor, c.s);
}
int bilinear_bwd(const Ctx& c, const Unit& u, Bwd& b) {
    VS_TRY(b.g.need(u.out));
    ProfScope prof(PK_POOL_MISC, 0, 1.25 * c.n * u.hout * u.wout * u.cout * c.net->esz, c.s);
    return vs_bilinear_up_bwd(c.net->dtype, c.da(u.out), c.da(u.src0), c.n, u.hin, u.win, u.cout, u.factor, b.g.next(u.src0), c.s);
}

// U_DROPOUT: nn.Dropout2d(0.2) in training, the identity in evaluation (smp FPNDecoder.dropout)
int dropout_fwd(const Ctx& c, const Unit& u, Fwd& f) {
    const vs_unet* net = c.net;
    const int dt = net->dtype;
    ProfScope prof(PK_POOL_MISC, 0, 2.0 * c.n * u.hout * u.wout * u.cout * net->esz, c.s);
    if (!f.training) return vs_channel_slice(dt, c.a(u.src0), u.cout, 0, c.a(u.out), u.cout, 0, u.cout, c.rows(u), 0, c.s);
    float* mask = (float*)(c.ws + net->off_dropmask);
    VS_TRY(vs_dropout2d_mask(mask, c.n, u.cout, 0.2f, net->rng_seed, net->rng_counter, 0, c.s));
    return vs_channel_scale(dt, c.a(u.src0), mask, c.a(u.out), c.n, (int64_t)u.hout * u.wout, u.cout, c.s);
}
int dropout_bwd(const Ctx& c, const Unit& u, Bwd& b) {
    const vs_unet* net = c.net;
    VS_TRY(b.g.need(u.out));
    VS_TRY(b.g.first(u.src0));
    ProfScope prof(PK_POOL_MISC, 0, 2.0 * c.n * u.hout * u.wout * u.cout * net->esz, c.s);
    return vs_channel_scale(net->dtype, c.da(u.out), (const float*)(c.ws + net->off_dropmask), c.da(u.src0), c.n, (int64_t)u.hout * u.wout, u.cout, c.s);
}

// U_DWCONV: depthwise 3x3 convolution, dilation = padding = dil (first half of smp's SeparableConv2d), no norm
int dwconv_fwd(const Ctx& c, const Unit& u, Fwd&) {
    ProfScope prof(PK_POOL_MISC, 0, 2.0 * c.n * u.hout * u.wout * u.cout * c.net->esz, c.s);
    return vs_dwconv3x3(c.net->dtype, c.a(u.src0), c.P(u.w_idx), c.a(u.out), c.n, u.hin, u.win, u.cout, u.dil, 0, c.s);
}
int dwconv_bwd_norm(const Ctx&, const Unit& u, Bwd& b) { return b.g.need(u.out); }    // (U_DWCONV2 too)
int dwconv_bwd_data(const Ctx& c, const Unit& u, Bwd& b, Dz dz) {   // the same sweep, taps reversed
    ProfScope prof(PK_CONV_DGRAD, 2.0 * c.n * u.hout * u.wout * u.cout * 9, 0, c.s);
    return vs_dwconv3x3(c.net->dtype, dz.p, c.P(u.w_idx), c.da(u.src0), c.n, u.hin, u.win, u.cout, u.dil, 1 | (b.g.next(u.src0) ? 2 : 0), c.s);
}
int dwconv_wgrad(const Ctx& c, const Unit& u, const Bwd& b, Dz dz, hipStream_t s, int slab) {
    ProfScope prof(PK_CONV_WGRAD, 2.0 * c.n * u.hout * u.wout * u.cout * 9, 0, s);
    return vs_dwconv3x3_wgrad(c.net->dtype, c.a(u.src0), dz.p, b.grad(c, u.w_idx), c.n, u.hin, u.win, u.cout, u.dil, c.wgws(slab), c.net->wgws_bytes, (void*)s);
}

// U_GAP: nn.AdaptiveAvgPool2d(1): out [n][1][1][c]
int gap_fwd(const Ctx& c, const Unit& u, Fwd&) {
    const vs_unet* net = c.net;
    ProfScope prof(PK_POOL_MISC, 0, (double)c.n * u.hin * u.win * u.cout * net->esz, c.s);
    return vs_sample_rowsum_ws(net->dtype, c.a(u.src0), nullptr, c.a(u.out), c.n, (int64_t)u.hin * u.win, u.cout, 1.f / (float)(u.hin * u.win),
                               (float*)(c.ws + net->off_gapws), net->gapws_bytes, c.s);
}
int gap_bwd(const Ctx& c, const Unit& u, Bwd& b) {      // every position receives the pooled gradient / hw
    VS_TRY(b.g.need(u.out));
    ProfScope prof(PK_POOL_MISC, 0, 2.0 * c.n * u.hin * u.win * u.cout * c.net->esz, c.s);
    return vs_broadcast_rows(c.net->dtype, c.da(u.out), c.da(u.src0), c.n, (int64_t)u.hin * u.win, u.cout, 1.f / (float)(u.hin * u.win), b.g.next(u.src0), c.s);
}

// U_BCAST: F.interpolate of a 1x1 map to hout x wout (ASPPPooling)
int bcast_fwd(const Ctx& c, const Unit& u, Fwd&) {
    ProfScope prof(PK_POOL_MISC, 0, (double)c.n * u.hout * u.wout * u.cout * c.net->esz, c.s);
    return vs_broadcast_rows(c.net->dtype, c.a(u.src0), c.a(u.out), c.n, (int64_t)u.hout * u.wout, u.cout, 1.f, 0, c.s);
}
int bcast_bwd(const Ctx& c, const Unit& u, Bwd& b) {    // the 1x1 map receives the sum over the positions it was copied to
    VS_TRY(b.g.need(u.out));
    VS_TRY(b.g.first(u.src0));
    ProfScope prof(PK_POOL_MISC, 0, (double)c.n * u.hout * u.wout * u.cout * c.net->esz, c.s);
    return vs_spatial_sum(c.net->dtype, c.da(u.out), c.da(u.src0), c.n, (int64_t)u.hout * u.wout, u.cout, 1.f, c.s);
}

// U_DROPOUT_E: element-wise nn.Dropout(0.5) (ASPP.project), the identity in evaluation; the backward draws the same mask again
int dropout_e_fwd(const Ctx& c, const Unit& u, Fwd& f) {
    const vs_unet* net = c.net;
    ProfScope prof(PK_POOL_MISC, 0, 2.0 * c.n * u.hout * u.wout * u.cout * net->esz, c.s);
    if (!f.training) return vs_channel_slice(net->dtype, c.a(u.src0), u.cout, 0, c.a(u.out), u.cout, 0, u.cout, c.rows(u), 0, c.s);
    return vs_dropout(net->dtype, c.a(u.src0), c.a(u.out), c.rows(u) * u.cout, 0.5f, net->rng_seed ^ 0x5bd1e995u, net->rng_counter, 0, c.s);
}
int dropout_e_bwd(const Ctx& c, const Unit& u, Bwd& b) {
    const vs_unet* net = c.net;
    VS_TRY(b.g.need(u.out));
    VS_TRY(b.g.first(u.src0));
    ProfScope prof(PK_POOL_MISC, 0, 2.0 * c.n * u.hout * u.wout * u.cout * net->esz, c.s);
    return vs_dropout(net->dtype, c.da(u.out), c.da(u.src0), c.rows(u) * u.cout, 0.5f, net->rng_seed ^ 0x5bd1e995u, net->rng_counter, 0, c.s);
}

// U_PAB: smp MAnet's PAB attention: out = src0 + reinterpret(softmax_all(center top^T) bottom); members = {top, center, bottom}
int pab_fwd(const Ctx& c, const Unit& u, Fwd&) {
    const vs_unet* net = c.net;
    ProfScope prof(PK_POOL_MISC, 0, 4.0 * c.n * u.hout * u.wout * u.cout * net->esz, c.s);
    return vs_pab_attention_fwd(net->dtype, c.a(u.members[0]), c.a(u.members[1]), c.a(u.members[2]), c.a(u.src0), c.a(u.out), (float*)(c.ws + u.off_gn),
                                (float*)(c.ws + net->off_pab), c.n, u.hout * u.wout, u.cin0, u.cout, c.s);
}
int pab_bwd(const Ctx& c, const Unit& u, Bwd& b) {      // identity path + the attention term's gradients w.r.t. its three convolution outputs
    const vs_unet* net = c.net;
    VS_TRY(b.g.need(u.out));
    for (int m : u.members) VS_TRY(b.g.first(m));
    ProfScope prof(PK_POOL_MISC, 0, 6.0 * c.n * u.hout * u.wout * u.cout * net->esz, c.s);
    VS_TRY(vs_channel_slice(net->dtype, c.da(u.out), u.cout, 0, c.da(u.src0), u.cout, 0, u.cout, c.rows(u), b.g.next(u.src0), c.s));
    return vs_pab_attention_bwd(net->dtype, c.da(u.out), c.a(u.members[0]), c.a(u.members[1]), c.a(u.members[2]), (const float*)(c.ws + u.off_gn),
                                c.da(u.members[0]), c.da(u.members[1]), c.da(u.members[2]), (float*)(c.ws + net->off_pab), c.n, u.hout * u.wout, u.cin0,
                                u.cout, c.s);
}

// U_SE: squeeze-excitation gate on a pooled [n][1][1][c] feature: tensors w_idx .. w_idx + 3 = W1, b1, W2, b2; cin1 = hidden width
int se_fwd(const Ctx& c, const Unit& u, Fwd&) {
    ProfScope prof(PK_POOL_MISC, 4.0 * c.n * u.cout * u.cin1, 0, c.s);
    return vs_se_gate_fwd(c.net->dtype, c.a(u.src0), c.P(u.w_idx), c.P(u.w_idx + 1), c.P(u.w_idx + 2), c.P(u.w_idx + 3), c.a(u.out),
                          (float*)(c.ws + u.off_gn), c.n, u.cout, u.cin1, u.relu == 2, c.s);
}
int se_bwd(const Ctx& c, const Unit& u, Bwd& b) {       // the gate's parameter gradients are produced here, on the caller's stream (a few hundred values)
    VS_TRY(b.g.need(u.out));
    VS_TRY(b.g.first(u.src0));
    ProfScope prof(PK_POOL_MISC, 12.0 * c.n * u.cout * u.cin1, 0, c.s);
    return vs_se_gate_bwd(c.net->dtype, c.da(u.out), c.a(u.out), c.a(u.src0), (const float*)(c.ws + u.off_gn), c.P(u.w_idx), c.P(u.w_idx + 2), c.da(u.src0),
                          b.grad(c, u.w_idx), b.grad(c, u.w_idx + 1), b.grad(c, u.w_idx + 2), b.grad(c, u.w_idx + 3), (float*)(c.ws + c.net->off_sews), c.n,
                          u.cout, u.cin1, u.relu == 2, c.s);
}

// U_CGATE: out = a(src0) * gate a(src1) ([n][1][1][c]) over the map
int cgate_fwd(const Ctx& c, const Unit& u, Fwd&) {
    ProfScope prof(PK_POOL_MISC, 0, 2.0 * c.n * u.hout * u.wout * u.cout * c.net->esz, c.s);
    return vs_channel_gate(c.net->dtype, c.a(u.src0), c.a(u.src1), c.a(u.out), c.n, (int64_t)u.hout * u.wout, u.cout, c.s);
}
int cgate_bwd(const Ctx& c, const Unit& u, Bwd& b) {    // d(input) = dy * gate, d(gate)[n][c] = sum over the map of dy * input
    const vs_unet* net = c.net;
    VS_TRY(b.g.need(u.out));
    VS_TRY(b.g.first(u.src0));
    VS_TRY(b.g.first(u.src1));
    ProfScope prof(PK_POOL_MISC, 0, 4.0 * c.n * u.hout * u.wout * u.cout * net->esz, c.s);
    VS_TRY(vs_sample_rowsum_ws(net->dtype, c.a(u.src0), c.da(u.out), c.da(u.src1), c.n, (int64_t)u.hout * u.wout, u.cout, 1.f, (float*)(c.ws + net->off_gapws),
                               net->gapws_bytes, c.s));
    return vs_channel_gate(net->dtype, c.da(u.out), c.a(u.src1), c.da(u.src0), c.n, (int64_t)u.hout * u.wout, u.cout, c.s);
}

// U_SIGMOID: element-wise sigmoid (smp PAN's GAU gate)
int sigmoid_fwd(const Ctx& c, const Unit& u, Fwd&) { return vs_sigmoid(c.net->dtype, c.a(u.src0), c.a(u.out), c.rows(u) * u.cout, c.s); }
int sigmoid_bwd(const Ctx& c, const Unit& u, Bwd& b) {
    VS_TRY(b.g.need(u.out));
    VS_TRY(b.g.first(u.src0));
    return vs_sigmoid_bwd(c.net->dtype, c.da(u.out), c.a(u.out), c.da(u.src0), c.rows(u) * u.cout, c.s);
}

// U_BN: standalone nn.BatchNorm2d(cout, bn_eps, bn_mom) + activation `relu` (0 none / 1 ReLU / 2 swish) on a(src0), any channel count
// (csrc/effnet.hip): the norms of smp's EfficientNet encoders.  Batch statistics (training) or the running ones, normalisation +
// activation in one sweep; where the convolution in front of it can take it into its epilogue (evaluation) the loop skips it.
int bn_fwd(const Ctx& c, const Unit& u, Fwd& f) {
    const vs_unet* net = c.net;
    const int dt = net->dtype;
    float *rm = c.rmean(u), *rv = c.rvar(u);
    ProfScope prof(f.training ? PK_BN_STATS : PK_BN_APPLY, 0, (f.training ? 3.0 : 2.0) * c.n * u.hout * u.wout * u.cout * net->esz, c.s);
    const int64_t rows = c.rows(u);
    if (!f.training) return vs_bn2_apply(dt, c.a(u.src0), rm, rv, c.P(u.bn_idx), c.P(u.bn_idx + 1), u.relu, u.bn_eps, c.a(u.out), rows, u.cout, c.s);
    if (f.carried_stat_rows) {
        VS_TRY(launch_bn_finalize_partials(c.bnws(), f.carried_stat_rows, u.cout, rows, u.bn_eps, u.bn_mom, c.bnc(u, 2), c.bnc(u, 3), rm, rv, c.s));
        f.carried_stat_rows = 0;
    } else {
        VS_TRY(vs_bn2_stats(dt, c.a(u.src0), rows, u.cout, u.bn_eps, u.bn_mom, c.bnc(u, 2), c.bnc(u, 3), rm, rv, c.bnws(), net->bnws_bytes, c.s));
    }
    return vs_bn2_apply(dt, c.a(u.src0), c.bnc(u, 2), c.bnc(u, 3), c.P(u.bn_idx), c.P(u.bn_idx + 1), u.relu, -1.f, c.a(u.out), rows, u.cout, c.s);
}
int bn_bwd(const Ctx& c, const Unit& u, Bwd& b) {       // dx, dgamma, dbeta; the activation's derivative is recomputed from the pre-norm tensor
    const vs_unet* net = c.net;
    VS_TRY(b.g.need(u.out));
    VS_TRY(b.g.first(u.src0));
    ProfScope prof(PK_BN_BWD, 0, 5.0 * c.n * u.hout * u.wout * u.cout * net->esz, c.s);
    return vs_bn2_bwd(net->dtype, c.da(u.out), c.a(u.src0), c.bnc(u, 2), c.bnc(u, 3), c.P(u.bn_idx), c.P(u.bn_idx + 1), u.relu, c.da(u.src0), b.grad(c, u.bn_idx),
                      b.grad(c, u.bn_idx + 1), c.rows(u), u.cout, c.bnws(), net->bnws_bytes, c.s);
}

// U_DWCONV2: depthwise k x k convolution, stride 1 / 2, `pad` zero rows / columns in front (static same padding), no norm; bcast: the
// network input (one fp32 channel) broadcast over cout = the EfficientNet stem
int dwconv2_fwd(const Ctx& c, const Unit& u, Fwd& f) {
    const vs_unet* net = c.net;
    const int dt = net->dtype, n = c.n;
    ProfScope prof(PK_POOL_MISC, 0, (double)n * (u.hin * u.win * u.cin0 + u.hout * u.wout * u.cout) * net->esz, c.s);
    const Unit* next_bn = bn_behind(net, f.ui);
    if (!f.training && !u.bcast && next_bn && (u.dil == 1 || (u.stride == 1 && (u.dil == 2 || (u.dil == 4 && u.k == 3))))) {
        const Unit& bn = *next_bn;      // evaluation: its BatchNorm (folded) + swish in the same sweep
        f.skip_units = 1;
        return vs_dwconv2d_affine(dt, c.a(u.src0), c.P(u.w_idx), c.bnc(bn, 0), c.bnc(bn, 1), bn.relu, c.a(bn.out), n, u.hin, u.win, u.cout, u.k, u.stride,
                                  u.pad, u.dil, u.hout, u.wout, c.s);
    }
    return vs_dwconv2d(dt, u.bcast ? (const void*)f.x : (const void*)c.a(u.src0), c.P(u.w_idx), c.a(u.out), n, u.hin, u.win, u.cout, u.k, u.stride, u.pad,
                       u.dil, u.hout, u.wout, u.bcast, c.s);
}
// (norm half: dwconv_bwd_norm)
int dwconv2_bwd_data(const Ctx& c, const Unit& u, Bwd& b, Dz dz) {   // none for the stem: its input is the network's
    if (u.bcast) return VS_OK;
    ProfScope prof(PK_CONV_DGRAD, 2.0 * c.n * u.hout * u.wout * u.cout * u.k * u.k, 0, c.s);
    return vs_dwconv2d_bwd_data(c.net->dtype, dz.p, c.P(u.w_idx), c.da(u.src0), c.n, u.hin, u.win, u.cout, u.k, u.stride, u.pad, u.dil, u.hout, u.wout,
                                b.g.next(u.src0), c.s);
}
int dwconv2_wgrad(const Ctx& c, const Unit& u, const Bwd& b, Dz dz, hipStream_t s, int slab) {
    const vs_unet* net = c.net;
    const bool want_w = b.want_w(u);
    ProfScope prof(PK_CONV_WGRAD, want_w ? 2.0 * c.n * u.hout * u.wout * u.cout * u.k * u.k : 0, 0, s);
    if (want_w)
        return vs_dwconv2d_wgrad(net->dtype, u.bcast ? (const void*)b.x : (const void*)c.a(u.src0), dz.p, b.grad(c, u.w_idx), c.n, u.hin, u.win, u.cout, u.k,
                                 u.stride, u.pad, u.dil, u.hout, u.wout, u.bcast, c.wgws(slab), net->wgws_bytes, (void*)s);
    VS_CHECK_HIP(hipMemsetAsync(b.grad(c, u.w_idx), 0, tensor_elems(c.t(u.w_idx)) * sizeof(float), s));
    return VS_OK;
}

// U_DROPADD: out = drop_connect(a(src0), drop_p) + a(src1) (the MBConv skip); evaluation: the plain sum.  salt = the block index
// (separates the blocks' draws)
int dropadd_fwd(const Ctx& c, const Unit& u, Fwd& f) {
    const vs_unet* net = c.net;
    ProfScope prof(PK_POOL_MISC, 0, 3.0 * c.n * u.hout * u.wout * u.cout * net->esz, c.s);
    const float* mask = nullptr;
    if (f.training && u.drop_p > 0.f) {
        float* m = (float*)(c.ws + u.off_gn);
        VS_TRY(vs_dropout2d_mask(m, c.n, 1, u.drop_p, net->rng_seed ^ 0x2545f491u, net->rng_counter, (int64_t)u.salt << 32, c.s));
        mask = m;
    }
    return vs_sample_scale_add(net->dtype, c.a(u.src0), mask, c.a(u.src1), c.a(u.out), c.n, (int64_t)u.hout * u.wout * u.cout, c.s);
}
int dropadd_bwd(const Ctx& c, const Unit& u, Bwd& b) {  // the skip takes the gradient as is, the block's branch the surviving samples' (scaled by 1 / keep)
    const vs_unet* net = c.net;
    VS_TRY(b.g.need(u.out));
    VS_TRY(b.g.first(u.src0));
    ProfScope prof(PK_POOL_MISC, 0, 4.0 * c.n * u.hout * u.wout * u.cout * net->esz, c.s);
    VS_TRY(vs_channel_slice(net->dtype, c.da(u.out), u.cout, 0, c.da(u.src1), u.cout, 0, u.cout, c.rows(u), b.g.next(u.src1), c.s));
    return vs_sample_scale_add(net->dtype, c.da(u.out), u.drop_p > 0.f ? (const float*)(c.ws + u.off_gn) : nullptr, nullptr, c.da(u.src0), c.n,
                               (int64_t)u.hout * u.wout * u.cout, c.s);
}

// U_FOLD2: out [.., c] = in [.., :c] + in [.., c:] (the sum over ResNeSt's two radix splits; maps and pooled vectors)
int fold2_fwd(const Ctx& c, const Unit& u, Fwd&) {
    const int dt = c.net->dtype;
    ProfScope prof(PK_POOL_MISC, 0, 3.0 * c.n * u.hout * u.wout * u.cout * c.net->esz, c.s);
    VS_TRY(vs_channel_slice(dt, c.a(u.src0), 2 * u.cout, 0, c.a(u.out), u.cout, 0, u.cout, c.rows(u), 0, c.s));
    return vs_channel_slice(dt, c.a(u.src0), 2 * u.cout, u.cout, c.a(u.out), u.cout, 0, u.cout, c.rows(u), 1, c.s);
}
int fold2_bwd(const Ctx& c, const Unit& u, Bwd& b) {    // both splits receive the sum's gradient
    const int dt = c.net->dtype;
    VS_TRY(b.g.need(u.out));
    ProfScope prof(PK_POOL_MISC, 0, 3.0 * c.n * u.hout * u.wout * u.cout * c.net->esz, c.s);
    const int acc = b.g.next(u.src0);
    VS_TRY(vs_channel_slice(dt, c.da(u.out), u.cout, 0, c.da(u.src0), 2 * u.cout, 0, u.cout, c.rows(u), acc, c.s));
    return vs_channel_slice(dt, c.da(u.out), u.cout, 0, c.da(u.src0), 2 * u.cout, u.cout, u.cout, c.rows(u), acc, c.s);
}

// U_RSOFTMAX: timm's RadixSoftmax(2, 1) on attention logits [n][2 c]
int rsoftmax_fwd(const Ctx& c, const Unit& u, Fwd&) { return vs_radix2_softmax(c.net->dtype, c.a(u.src0), c.a(u.out), c.n, u.cout / 2, c.s); }
int rsoftmax_bwd(const Ctx& c, const Unit& u, Bwd& b) {
    VS_TRY(b.g.need(u.out));
    VS_TRY(b.g.first(u.src0));
    return vs_radix2_softmax_bwd(c.net->dtype, c.da(u.out), c.a(u.out), c.da(u.src0), c.n, u.cout / 2, c.s);
}

// U_RADIXSUM: out [.., c] = a(src0)[.., :c] * gate[:c] + a(src0)[.., c:] * gate[c:], gate = a(src1) [n][2 c] (the attention-weighted sum of
// ResNeSt's two splits in one sweep)
int radixsum_fwd(const Ctx& c, const Unit& u, Fwd&) {
    ProfScope prof(PK_POOL_MISC, 0, 3.0 * c.n * u.hout * u.wout * u.cout * c.net->esz, c.s);
    return vs_radix2_gated_sum(c.net->dtype, c.a(u.src0), c.a(u.src1), c.a(u.out), c.n, (int64_t)u.hout * u.wout, u.cout, c.s);
}
int radixsum_bwd(const Ctx& c, const Unit& u, Bwd& b) { // d(splits) = dout * gate per split; d(gate)[n][r c + ch] = sum over the map of dout * split r
    const vs_unet* net = c.net;
    VS_TRY(b.g.need(u.out));
    VS_TRY(b.g.first(u.src0));
    VS_TRY(b.g.first(u.src1));
    ProfScope prof(PK_POOL_MISC, 0, 6.0 * c.n * u.hout * u.wout * u.cout * net->esz, c.s);
    VS_TRY(vs_sample_rowsum_b(net->dtype, c.a(u.src0), c.da(u.out), u.cout, c.da(u.src1), c.n, (int64_t)u.hout * u.wout, 2 * u.cout,
                              (float*)(c.ws + net->off_gapws), net->gapws_bytes, c.s));
    return vs_radix2_gated_sum_bwd(net->dtype, c.da(u.out), c.a(u.src1), c.da(u.src0), c.n, (int64_t)u.hout * u.wout, u.cout, c.s);
}

// U_AVGPOOL: nn.AvgPool2d(k, stride) of ResNeSt's avd (3, padding 1, zeros counted) / avg_down (2): a depthwise convolution with
// constant taps pool_w
const float* avgpool_taps(const Ctx& c, const Unit& u) { return (const float*)(c.ws + (u.k == 3 ? c.net->off_avgw9 : c.net->off_avgw4)); }
int avgpool_fwd(const Ctx& c, const Unit& u, Fwd&) {
    ProfScope prof(PK_POOL_MISC, 0, (double)c.n * (u.hin * u.win + u.hout * u.wout) * u.cout * c.net->esz, c.s);
    return vs_dwconv2d(c.net->dtype, c.a(u.src0), avgpool_taps(c, u), c.a(u.out), c.n, u.hin, u.win, u.cout, u.k, u.stride, u.pad, 1, u.hout, u.wout, 0, c.s);
}
int avgpool_bwd(const Ctx& c, const Unit& u, Bwd& b) {  // the adjoint of the constant-tap depthwise convolution
    VS_TRY(b.g.need(u.out));
    ProfScope prof(PK_POOL_MISC, 0, (double)c.n * (u.hin * u.win + u.hout * u.wout) * u.cout * c.net->esz, c.s);
    return vs_dwconv2d_bwd_data(c.net->dtype, c.da(u.out), avgpool_taps(c, u), c.da(u.src0), c.n, u.hin, u.win, u.cout, u.k, u.stride, u.pad, 1, u.hout,
                                u.wout, b.g.next(u.src0), c.s);
}

// U_UP2: out = nearest-x2 upsampling of a(src0), materialised - where a decoder's upsample + concat cannot ride the convolution's
// loader (the boundary is not a multiple of 32 channels: EfficientNet features of 136 / 56 / 48)
int up2_fwd(const Ctx& c, const Unit& u, Fwd&) {
    ProfScope prof(PK_POOL_MISC, 0, 1.25 * c.n * u.hout * u.wout * u.cout * c.net->esz, c.s);
    return vs_upsample2x_add(c.net->dtype, c.a(u.src0), nullptr, c.a(u.out), c.n, u.hin, u.win, u.cout, c.s);
}
int up2_bwd(const Ctx& c, const Unit& u, Bwd& b) {      // the 2x2 sums of the upsampled tensor's gradient
    VS_TRY(b.g.need(u.out));
    ProfScope prof(PK_POOL_MISC, 0, 1.25 * c.n * u.hout * u.wout * u.cout * c.net->esz, c.s);
    return launch_upsample2x_bwd(c.net->dtype, c.da(u.out), c.da(u.src0), c.n, u.hin, u.win, u.cout, b.g.next(u.src0), c.s);
}

// U_FPA: smp PAN's FPABlock pyramid + combination: out = plane(src0) * a(src1) + a(res) broadcast; tens = its 24 parameter tensors
// (6 x conv weight, conv bias, BN gamma, BN beta).  Max-pool, 7x7 convolution to the first single-channel map, the pyramid (one
// workgroup), the combination
int fpa_fwd(const Ctx& c, const Unit& u, Fwd& f) {
    const vs_unet* net = c.net;
    const int dt = net->dtype, n = c.n;
    ProfScope prof(PK_POOL_MISC, 0, 3.0 * n * u.hin * u.win * u.cin0 * net->esz, c.s);
    float* arena = (float*)(c.ws + u.off_fpa_arena);
    float* plane = (float*)(c.ws + u.off_fpa_plane);
    VS_TRY(vs_maxpool2x2(dt, c.a(u.src0), c.ws + u.off_fpa_pool, n, u.hin, u.win, u.cin0, c.s));
    VS_TRY(vs_conv_to_plane(dt, c.ws + u.off_fpa_pool, c.P(u.tens[0]), c.P(u.tens[1]), arena, n, u.hin / 2, u.win / 2, u.cin0, 7, c.s));
    float* pp[36];
    for (int i = 0; i < 6; ++i) {
        for (int j = 0; j < 4; ++j) pp[6 * i + j] = const_cast<float*>(c.P(u.tens[4 * i + j]));
        pp[6 * i + 4] = c.bnstate + c.t(u.tens[4 * i + 2] + 2).offset; pp[6 * i + 5] = c.bnstate + c.t(u.tens[4 * i + 2] + 3).offset;
    }
    VS_TRY(vs_fpa_pyramid_fwd(arena, plane, pp, n, u.hin, u.win, f.training ? 1 : 0, c.s));
    return vs_fpa_combine(dt, plane, c.a(u.src1), c.a(u.res), c.a(u.out), n, (int64_t)u.hout * u.wout, u.cout, c.s);
}
int fpa_bwd(const Ctx& c, const Unit& u, Bwd& b) {      // everything on the caller's stream (tiny): combination, pooled branch, pyramid, 7x7 convolution, max-pool
    const vs_unet* net = c.net;
    const int dt = net->dtype, n = c.n;
    VS_TRY(b.g.need(u.out));
    VS_TRY(b.g.first(u.src1));
    VS_TRY(b.g.first(u.res));
    ProfScope prof(PK_POOL_MISC, 0, 4.0 * n * u.hin * u.win * u.cin0 * net->esz, c.s);
    float* arena = (float*)(c.ws + u.off_fpa_arena);
    float* plane = (float*)(c.ws + u.off_fpa_plane);
    float* dplane = plane + (size_t)n * u.hin * u.win;
    VS_TRY(vs_fpa_combine_bwd(dt, c.da(u.out), plane, c.a(u.src1), c.da(u.src1), dplane, n, (int64_t)u.hout * u.wout, u.cout, c.s));
    VS_TRY(vs_spatial_sum(dt, c.da(u.out), c.da(u.res), n, (int64_t)u.hout * u.wout, u.cout, 1.f, c.s));
    float* pp[36]; float* gp[24];
    for (int i = 0; i < 6; ++i) {
        for (int j = 0; j < 4; ++j) { pp[6 * i + j] = const_cast<float*>(c.P(u.tens[4 * i + j])); gp[4 * i + j] = b.grad(c, u.tens[4 * i + j]); }
        pp[6 * i + 4] = nullptr; pp[6 * i + 5] = nullptr;       // running statistics are not touched by the backward pass
    }
    VS_TRY(vs_fpa_pyramid_bwd(arena, dplane, pp, gp, n, u.hin, u.win, c.s));
    // down1's convolution: its weight / bias gradients overwrite slots 0 / 1 (the pyramid kernel leaves them alone)
    char* dpool = c.ws + u.off_fpa_pool + (size_t)n * (u.hin / 2) * (u.win / 2) * u.cin0 * net->esz;
    VS_TRY(vs_conv_to_plane_bwd(dt, c.ws + u.off_fpa_pool, c.P(u.tens[0]), arena + vs_fpa_dz1_offset(n, u.hin, u.win), dpool, b.grad(c, u.tens[0]),
                                b.grad(c, u.tens[1]), n, u.hin / 2, u.win / 2, u.cin0, 7, c.s));
    return vs_maxpool2x2_bwd(dt, c.a(u.src0), dpool, c.da(u.src0), n, u.hin, u.win, u.cin0, b.g.next(u.src0), c.s);
}

// The weight gradient of a weighted unit on stream s, with the slab buffer number `slab`
int unit_wgrad(const Ctx& c, const Unit& u, const Bwd& b, Dz dz, hipStream_t s, int slab) {
    switch (u.kind) {
    case U_STEM:    return stem_wgrad(c, u, b, dz, s, slab);
    case U_CONV:    return conv_wgrad(c, u, b, dz, s, slab);
    case U_CONVT:   return conv_wgrad(c, u, b, dz, s, slab);
    case U_HEAD:    return conv_wgrad(c, u, b, dz, s, slab);
    case U_DWCONV:  return dwconv_wgrad(c, u, b, dz, s, slab);
    case U_DWCONV2: return dwconv2_wgrad(c, u, b, dz, s, slab);
    default:        return VS_OK;
    }
}

// unit index -> does an optimiser group of the fused backward start here (built once).  The network is cut into groups (decoder +
// head, layer4, layer3, layer2, layer1, stem).
void ensure_group_first(vs_unet* net) {
    if (!net->group_first.empty()) return;
    static const char* const kCuts[] = {"decoder.", "encoder.layer4.0.", "encoder.layer3.0.", "encoder.layer2.0.", "encoder.layer1.0."};
    const int ncuts = 5;                                  // (the stem is a group of its own: layer1's update then runs under the max-pool /
    net->group_first.assign(net->units.size(), 0);        // stem BatchNorm backward instead of behind the stem's gradient - 0.03 ms per step)
    net->group_first[0] = 1;
    std::string prev;
    for (size_t k = 0; k < net->units.size(); ++k) {
        if (net->units[k].w_idx < 0) continue;
        const std::string& nm = net->layout.tensors[net->units[k].w_idx].name;
        for (int ci = 0; ci < ncuts; ++ci)
            if (nm.rfind(kCuts[ci], 0) == 0 && prev.rfind(kCuts[ci], 0) != 0) net->group_first[k] = 1;
        prev = nm;
    }
}

// role: which stream's share of the work a call enqueues.  ROLE_BOTH is the normal two-stream form (fork / join events
// inside: struct SideWork).  ROLE_MAIN / ROLE_SIDE enqueue only the caller's-stream kernels / only the weight-gradient + optimiser kernels,
// both on `stream`: a recorded step keeps each share as its own LINEAR hipGraph (the runtime replays a linear graph of
// kernels as one batch of queue packets - 0.13 ms of host time per step - but walks a graph with parallel branches node by
// node, slower than launching call by call).  The split roles use no events: the caller orders the two shares itself, range
// by range (hipEventRecordWithFlags(hipEventRecordExternal), which would let ONE pair of graphs carry the fork events as
// external event nodes, returns hipErrorInvalidValue under capture on ROCm 7.2).
enum { ROLE_BOTH = 0, ROLE_MAIN = 1, ROLE_SIDE = 2 };

// The weight-gradient share of one backward call: which units' weight gradients wait for a fork event, the stream and slab buffer
// they run on, and the fused optimiser step behind them.  ROLE_BOTH with the side_stream option: forked from / joined to the
// caller's stream by events; otherwise everything in order on the caller's stream (ROLE_MAIN enqueues none of it).
struct SideWork {
    const Ctx& c;
    const Bwd& b;
    vs_unet* const net;
    const int role;
    const int n_side;              // side streams in use (0: none)
    const int fork_every;          // one fork event covers the weight gradients of up to this many consecutive units
    // The stem is the last unit of the backward pass: behind its BatchNorm backward the caller's stream has nothing left
    // to do but wait for the side stream, which still owes layer1's last weight gradients and their update.  With the fused
    // optimiser step the stem's weight gradient and update (a group of its own) therefore run on the CALLER's stream, beside
    // that tail instead of behind it (second slab workspace; profiles/r4_ab_side_stream_experiments.log).
    const bool stem_on_caller;
    bool side_used[vs_unet::kSide] = {false, false};   // side streams this call forked onto (only those are joined: under
                                                       // stream capture a stream that never joined the capture must not be waited on)
    struct Item { int ui; Dz dz; };
    std::vector<Item> pending;     // weighted units whose dz is (being) produced and whose weight gradient is not yet queued

    SideWork(const Ctx& c_, const Bwd& b_, int role_)
        : c(c_), b(b_), net(c_.net), role(role_), n_side(role_ == ROLE_BOTH ? vs_option("side_stream") : 0),
          fork_every(std::max(1, vs_option("fork_every"))), stem_on_caller(n_side > 0 && b_.opt) {}

    int setup() {
        if (b.opt) ensure_group_first(net);
        if (n_side <= 0) return VS_OK;
        // (a lowest-priority side stream was measured: 4.843 vs 4.853 ms per step - no preference of the dispatcher to speak of)
        VS_TRY(acquire_side_streams(net, c.s));
        for (int i = 0; i < vs_unet::kSide; ++i)
            if (!net->join_event[i]) VS_CHECK_HIP(hipEventCreateWithFlags(&net->join_event[i], hipEventDisableTiming));
        while (net->fork_events.size() < net->units.size()) {
            hipEvent_t e;
            VS_CHECK_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            net->fork_events.push_back(e);
        }
        return VS_OK;
    }
    // The fork policy: one event (a barrier packet on the caller's stream, ~7 us of command-processor time) covers the
    // weight-gradient work of up to `fork_every` consecutive units.  True: fork and release now.
    // (releasing the head's weight gradient at once - its operands exist before the backward pass starts - was measured: 4.512 vs 4.477 ms, not kept)
    // (joining the side stream after every unit, or releasing a weight gradient only behind its unit's data gradient, were both
    // measured slower - 6.0 ms per step - and are not kept)
    bool push(int ui, Dz dz, bool last) {
        pending.push_back(Item{ui, dz});
        return (int)pending.size() >= fork_every || last;
    }
    int fork(int ui) {   // everything enqueued on the caller's stream so far happens-before the side work: dz of every pending unit is complete
        if (n_side > 0) VS_CHECK_HIP(hipEventRecord(net->fork_events[ui], c.s));
        return VS_OK;
    }
    // queues the weight gradients of the pending units behind the fork event of unit ui
    int release(int ui) {
        if (role != ROLE_MAIN) {
            hipStream_t s = c.s;
            int slab = 0;
            if (n_side > 0) {
                slab = (n_side >= 2 && !b.opt) ? (ui & 1) : 0;   // the fused optimiser step relies on ONE side stream's order
                s = net->side[slab];
                side_used[slab] = true;
                VS_CHECK_HIP(hipStreamWaitEvent(s, net->fork_events[ui], 0));
            }
            for (const Item& it : pending) {
                const bool on_caller = stem_on_caller && net->units[it.ui].kind == U_STEM;
                VS_TRY(wgrad_and_update(it, on_caller ? c.s : s, on_caller ? 1 : slab));
            }
        }
        pending.clear();
        prof_set_tag(ui);
        return VS_OK;
    }
    // Fused optimiser step: when the first unit of a group has queued its weight gradient, every gradient of the group is complete
    // in that stream's order (its BN / bias gradients were produced on the caller's stream before that unit's fork event), so ONE
    // AdamW launch over the group's parameter slice and ONE launch deriving its weight copies for the next forward follow there.
    int wgrad_and_update(const Item& it, hipStream_t s, int slab) {
        prof_set_tag(it.ui);
        VS_TRY(unit_wgrad(c, net->units[it.ui], b, it.dz, s, slab));
        if (!b.opt || !net->group_first[it.ui]) return VS_OK;
        int hi = it.ui + 1;   // the group is [ui, hi): up to the next group's first unit (or the end of the network)
        while (hi < (int)net->units.size() && !net->group_first[hi]) ++hi;
        return update_units(c, it.ui, hi, b.need_encoder_wgrad, b.grads, *b.opt, s);
    }
    int join() {  // the caller's stream continues only after every weight gradient is in place
        for (int i = 0; i < vs_unet::kSide; ++i) {
            if (n_side <= 0 || !side_used[i]) continue;
            VS_CHECK_HIP(hipEventRecord(net->join_event[i], net->side[i]));
            VS_CHECK_HIP(hipStreamWaitEvent(c.s, net->join_event[i], 0));
        }
        return VS_OK;
    }
};

}  // namespace

// ---- the loops ---------------------------------------------------------------------------------------
static int unet_forward(vs_unet_t* net, const float* params, float* bnstate, const float* x, int n, int training,
                        float* logits, void* workspace, void* stream, const VolScatter* scatter) {
    VS_REQUIRE(net && params && bnstate && x && logits && workspace, "unet_forward: null pointer");
    VS_REQUIRE(n >= 1 && n <= net->max_batch, "unet_forward: batch %d exceeds the plan's max_batch %d", n, net->max_batch);
    VS_REQUIRE(!(training && net->dtype == VS_F16), "unet_forward: fp16 is the inference precision (batch statistics, the backward pass and the optimiser are built for fp32 / bf16)");
    Ctx c{net, (char*)workspace, params, bnstate, (hipStream_t)stream, n};
    Fwd f{x, logits, training, scatter};
    net->last_n = n;
    net->nl_act.assign(net->acts.size(), 0);
    if (training && net->dtype == VS_BF16 && net->bins_bytes && vs_option("stats_bins"))
        VS_TRY(launch_zero_u64((unsigned long long*)(c.ws + net->off_bins0), net->bins_bytes / sizeof(unsigned long long), c.s));
    for (f.ui = 0; f.ui < (int)net->units.size(); ++f.ui) {
        const Unit& u = net->units[f.ui];
        prof_set_tag(f.ui);
        if (f.skip_units) { --f.skip_units; continue; }
        switch (u.kind) {
        case U_STEM:      VS_TRY(stem_fwd(c, u, f)); break;
        case U_POOL:      VS_TRY(pool_fwd(c, u, f)); break;
        case U_CONV:      VS_TRY(conv_fwd(c, u, f)); break;
        case U_HEAD:      VS_TRY(head_fwd(c, u, f)); break;
        case U_CONCAT:    VS_TRY(concat_fwd(c, u, f)); break;
        case U_CONVT:     VS_TRY(convt_fwd(c, u, f)); break;
        case U_ADD:       VS_TRY(add_fwd(c, u, f)); break;
        case U_UPADD:     VS_TRY(upadd_fwd(c, u, f)); break;
        case U_BILINEAR:  VS_TRY(bilinear_fwd(c, u, f)); break;
        case U_DROPOUT:   VS_TRY(dropout_fwd(c, u, f)); break;
        case U_DWCONV:    VS_TRY(dwconv_fwd(c, u, f)); break;
        case U_GAP:       VS_TRY(gap_fwd(c, u, f)); break;
        case U_BCAST:     VS_TRY(bcast_fwd(c, u, f)); break;
        case U_DROPOUT_E: VS_TRY(dropout_e_fwd(c, u, f)); break;
        case U_PAB:       VS_TRY(pab_fwd(c, u, f)); break;
        case U_SE:        VS_TRY(se_fwd(c, u, f)); break;
        case U_CGATE:     VS_TRY(cgate_fwd(c, u, f)); break;
        case U_SIGMOID:   VS_TRY(sigmoid_fwd(c, u, f)); break;
        case U_BN:        VS_TRY(bn_fwd(c, u, f)); break;
        case U_DWCONV2:   VS_TRY(dwconv2_fwd(c, u, f)); break;
        case U_DROPADD:   VS_TRY(dropadd_fwd(c, u, f)); break;
        case U_FOLD2:     VS_TRY(fold2_fwd(c, u, f)); break;
        case U_RSOFTMAX:  VS_TRY(rsoftmax_fwd(c, u, f)); break;
        case U_RADIXSUM:  VS_TRY(radixsum_fwd(c, u, f)); break;
        case U_AVGPOOL:   VS_TRY(avgpool_fwd(c, u, f)); break;
        case U_UP2:       VS_TRY(up2_fwd(c, u, f)); break;
        case U_FPA:       VS_TRY(fpa_fwd(c, u, f)); break;
        }
    }
    return (scatter && !f.head_scattered) ? 1 : VS_OK;   // 1: the caller still has to turn the logits into volume entries
}

static int unet_backward_range(vs_unet_t* net, const float* params, const float* x, const float* dlogits, int n,
                               int need_encoder_wgrad, float* grads, void* workspace, void* stream, int unit_lo, int unit_hi,
                               const vs_adamw_args* opt, int role = ROLE_BOTH) {
    VS_REQUIRE(net && params && x && dlogits && grads && workspace, "unet_backward: null pointer");
    VS_NO_F16(net->dtype, "unet_backward");
    const bool do_main = role != ROLE_SIDE;
    VS_REQUIRE(n == net->last_n, "unet_backward: batch %d does not match the last training forward (%d)", n, net->last_n);
    Ctx c{net, (char*)workspace, params, nullptr, (hipStream_t)stream, n};
    if (do_main && unit_hi == (int)net->units.size()) net->written.assign(net->acts.size(), 0);  // a new backward pass starts at the top
    ensure_graph_maps(net);
    if (do_main && unit_hi == (int)net->units.size()) net->bwd_stat_rows.assign(net->acts.size(), 0);
    VS_REQUIRE(net->written.size() == net->acts.size(), "unet_backward_range: ranges must start at the last unit");
    Bwd b{x, dlogits, grads, need_encoder_wgrad != 0, opt, Ledger{net->written}};
    SideWork side(c, b, role);
    VS_TRY(side.setup());
    for (int ui = unit_hi - 1; ui >= unit_lo; --ui) {
        const Unit& u = net->units[ui];
        prof_set_tag(ui);
        b.g.ui = ui; b.g.kind = u.kind;
        const bool weighted = u.kind == U_STEM || u.kind == U_CONV || u.kind == U_CONVT || u.kind == U_HEAD || u.kind == U_DWCONV || u.kind == U_DWCONV2;
        if (!weighted && !do_main) continue;      // the other kinds' work is all the caller's stream's
        switch (u.kind) {
        case U_POOL:      VS_TRY(pool_bwd(c, u, b)); continue;
        case U_CONCAT:    VS_TRY(concat_bwd(c, u, b)); continue;
        case U_ADD:       VS_TRY(add_bwd(c, u, b)); continue;
        case U_UPADD:     VS_TRY(upadd_bwd(c, u, b)); continue;
        case U_BILINEAR:  VS_TRY(bilinear_bwd(c, u, b)); continue;
        case U_DROPOUT:   VS_TRY(dropout_bwd(c, u, b)); continue;
        case U_GAP:       VS_TRY(gap_bwd(c, u, b)); continue;
        case U_BCAST:     VS_TRY(bcast_bwd(c, u, b)); continue;
        case U_DROPOUT_E: VS_TRY(dropout_e_bwd(c, u, b)); continue;
        case U_PAB:       VS_TRY(pab_bwd(c, u, b)); continue;
        case U_SE:        VS_TRY(se_bwd(c, u, b)); continue;
        case U_CGATE:     VS_TRY(cgate_bwd(c, u, b)); continue;
        case U_SIGMOID:   VS_TRY(sigmoid_bwd(c, u, b)); continue;
        case U_BN:        VS_TRY(bn_bwd(c, u, b)); continue;
        case U_DROPADD:   VS_TRY(dropadd_bwd(c, u, b)); continue;
        case U_FOLD2:     VS_TRY(fold2_bwd(c, u, b)); continue;
        case U_RSOFTMAX:  VS_TRY(rsoftmax_bwd(c, u, b)); continue;
        case U_RADIXSUM:  VS_TRY(radixsum_bwd(c, u, b)); continue;
        case U_AVGPOOL:   VS_TRY(avgpool_bwd(c, u, b)); continue;
        case U_UP2:       VS_TRY(up2_bwd(c, u, b)); continue;
        case U_FPA:       VS_TRY(fpa_bwd(c, u, b)); continue;
        default:          break;                  // the weighted kinds: norm half, fork, data gradient, weight gradient released
        }
        if (do_main) switch (u.kind) {
        case U_STEM:      VS_TRY(stem_bwd_norm(c, u, b)); break;
        case U_CONV:      VS_TRY(conv_bwd_norm(c, u, b)); break;
        case U_CONVT:     VS_TRY(convt_bwd_norm(c, u, b)); break;
        case U_HEAD:      VS_TRY(head_bwd_norm(c, u, b)); break;
        case U_DWCONV:    VS_TRY(dwconv_bwd_norm(c, u, b)); break;
        case U_DWCONV2:   VS_TRY(dwconv_bwd_norm(c, u, b)); break;
        default:          break;
        }
        const Dz dz = unit_dz(c, u);
        const bool flush = side.push(ui, dz, ui == unit_lo || u.kind == U_STEM);
        if (flush && do_main) VS_TRY(side.fork(ui));
        if (do_main) switch (u.kind) {            // (queued before the side-stream work so the caller's stream is fed first)
        case U_CONV:      VS_TRY(conv_bwd_data(c, u, b, dz)); break;
        case U_CONVT:     VS_TRY(conv_bwd_data(c, u, b, dz)); break;
        case U_HEAD:      VS_TRY(head_bwd_data(c, u, b, dz)); break;
        case U_DWCONV:    VS_TRY(dwconv_bwd_data(c, u, b, dz)); break;
        case U_DWCONV2:   VS_TRY(dwconv2_bwd_data(c, u, b, dz)); break;
        default:          break;                  // U_STEM: its input is the network's
        }
        if (flush) VS_TRY(side.release(ui));
    }
    if (!side.pending.empty()) {   // a range that ends on a unit without weights (the max-pool)
        const int ui = side.pending.back().ui;
        if (do_main) VS_TRY(side.fork(ui));
        VS_TRY(side.release(ui));
    }
    VS_TRY(side.join());
    if (opt && role == ROLE_BOTH) net->wset ^= 1;   // split roles: the caller flips once both shares are queued (vs_unet_flip_weight_set)
    return VS_OK;
}

// ---- prepare ---------------------------------------------------------------------------------------
extern "C" int vs_unet_prepare(vs_unet_t* net, const float* params, const float* bnstate, int training, void* workspace,
                               void* stream) {
    VS_REQUIRE(net && params && bnstate && workspace, "unet_prepare: null pointer");
    Ctx c{net, (char*)workspace, params, const_cast<float*>(bnstate), (hipStream_t)stream, 0};
    ProfScope prof(PK_PREPARE, 0, (double)net->layout.n_params * (4 + net->esz * (training ? 2 : 1)), c.s);
    VS_CHECK_HIP(hipMemsetAsync(c.ws + net->off_bncnt, 0, 256, c.s));   // (reserved, unused bytes of the plan: see unet_plan.h)
    {   // every conv layer's low-precision copy and flipped/transposed dgrad copy in one launch
        WeightCopyRow rows[64];
        int nl = 0;
        auto flush = [&]() -> int {
            if (!nl) return VS_OK;
            const int rc = launch_weight_prepare_all(net->dtype, params, c.ws, rows, nl, c.s);
            nl = 0;
            return rc;
        };
        for (auto& u : net->units) {
            if (u.kind != U_CONV && u.kind != U_HEAD) continue;
            rows[nl] = weight_copy_row(net, u, net->wset, training != 0, false);
            if (rows[nl].wc_off < 0 && rows[nl].wt_off < 0) continue;
            if (++nl == 64) {   // the descriptor table of one launch holds 64 layers (U-Net++ / resnet50 has 83)
                int rc = flush();
                if (rc) return rc;
            }
        }
        {
            int rc = flush();
            if (rc) return rc;
        }
        for (auto& u : net->units) {
            if (u.kind != U_CONVT) continue;
            const int rc = launch_convt_weight_prepare(net->dtype, c.P(u.w_idx), c.ws + Ctx::wc_off(u, net->wset),
                                                       training ? c.ws + Ctx::wt_off(u, net->wset) : nullptr, u.cin0, u.cout, c.s);
            if (rc) return rc;
        }
    }
    if (net->avgw_c) {     // the average pools' constant taps (the workspace may be a fresh allocation)
        const float w9 = 1.f / 9.f, w4 = 0.25f;
        VS_CHECK_HIP(hipMemsetD32Async((hipDeviceptr_t)(c.ws + net->off_avgw9), *reinterpret_cast<const int*>(&w9), (size_t)net->avgw_c * 9, c.s));
        VS_CHECK_HIP(hipMemsetD32Async((hipDeviceptr_t)(c.ws + net->off_avgw4), *reinterpret_cast<const int*>(&w4), (size_t)net->avgw_c * 4, c.s));
    }
    for (auto& u : net->units) {
        if (u.bn_idx >= 0 && !training) {  // eval-mode folding from the running statistics
            const float* rm = bnstate + c.t(u.bn_idx + 2).offset;
            const float* rv = bnstate + c.t(u.bn_idx + 3).offset;
            int rc = vs_bn_fold(c.P(u.bn_idx), c.P(u.bn_idx + 1), rm, rv, u.kind == U_BN ? u.bn_eps : 1e-5f, c.bnc(u, 0), c.bnc(u, 1), u.cout, stream);
            if (rc) return rc;
            if (u.kind == U_CONV && u.bias_idx >= 0 && (rc = vs_bn_fold_bias(c.bnc(u, 0), c.P(u.bias_idx), c.bnc(u, 1), u.cout, stream))) return rc;
        }
    }
    return VS_OK;
}

// Data-parallel form of the fused optimiser step (the caller all-reduces a bucket of gradients, updates that slice of the
// parameters and then calls this): weight copies of the units [unit_lo, unit_hi) into the plan's OTHER weight set;
// vs_unet_flip_weight_set makes that set current once every range has been refreshed.
extern "C" int vs_unet_prepare_range(vs_unet_t* net, const float* params, void* workspace, void* stream, int unit_lo, int unit_hi) {
    VS_REQUIRE(net && params && workspace && unit_lo >= 0 && unit_lo < unit_hi && unit_hi <= (int)net->units.size(),
               "unet_prepare_range: bad arguments");
    WeightCopyRow rows[64];
    int nl = 0;
    const int other = net->wset ^ 1;
    for (int k = unit_lo; k < unit_hi; ++k) {
        const Unit& v = net->units[k];
        if (v.kind == U_CONVT) {
            const int rc = launch_convt_weight_prepare(net->dtype, params + net->layout.tensors[v.w_idx].offset, (char*)workspace + Ctx::wc_off(v, other),
                                                       (char*)workspace + Ctx::wt_off(v, other), v.cin0, v.cout, (hipStream_t)stream);
            if (rc) return rc;
        }
        if (v.kind != U_CONV && v.kind != U_HEAD) continue;
        VS_REQUIRE(nl < 64, "unet_prepare_range: too many layers in one range");
        rows[nl++] = weight_copy_row(net, v, other, true, false);
    }
    if (!nl) return VS_OK;
    return launch_weight_prepare_all(net->dtype, params, workspace, rows, nl, (hipStream_t)stream);
}
extern "C" int vs_unet_weight_set(const vs_unet_t* net) { return net ? net->wset : VS_ERR_INVALID; }
// Dropout2d draws of a training forward (smp.FPN): mask = f(seed, *counter) with the counter in device memory (int64; the
// engine passes a BatchNorm's num_batches_tracked, which the training step advances) - a replayed graph draws a new mask per step
extern "C" int vs_unet_set_rng(vs_unet_t* net, uint32_t seed, const int64_t* counter) {
    VS_REQUIRE(net, "unet_set_rng: null pointer");
    net->rng_seed = seed; net->rng_counter = counter;
    return VS_OK;
}
extern "C" int vs_unet_side_stream(vs_unet_t* net, void* stream, int index, void** side) {
    VS_REQUIRE(net && side && index >= 0 && index < vs_unet::kSide, "unet_side_stream: bad arguments");
    const int rc = acquire_side_streams(net, (hipStream_t)stream);
    if (rc) return rc;
    *side = (void*)net->side[index];
    return VS_OK;
}

extern "C" int vs_unet_side_stream_overlaps(vs_unet_t* net, void* stream, int* overlaps) {
    VS_REQUIRE(net && overlaps, "unet_side_stream_overlaps: null pointer");
    int rc = acquire_side_streams(net, (hipStream_t)stream);
    if (rc) return rc;
    bool yes = false;
    if ((rc = streams_overlap((hipStream_t)stream, net->side[0], &yes))) return rc;
    *overlaps = yes ? 1 : 0;
    return VS_OK;
}

extern "C" int vs_unet_flip_weight_set(vs_unet_t* net) {
    VS_REQUIRE(net, "unet_flip_weight_set: null pointer");
    net->wset ^= 1;
    return VS_OK;
}

// ---- forward ---------------------------------------------------------------------------------------
extern "C" int vs_unet_forward(vs_unet_t* net, const float* params, float* bnstate, const float* x, int n, int training,
                               float* logits, void* workspace, void* stream) {
    VS_REQUIRE(logits, "unet_forward: null pointer");
    return unet_forward(net, params, bnstate, x, n, training, logits, workspace, stream, nullptr);
}

// Prediction: eval-mode forward whose segmentation head writes straight into the output volume(s) - the fused form of
// vs_unet_forward(training = 0) + vs_logits_to_volume (same arithmetic in the same order: identical labels, probabilities
// and keys).  Falls back to exactly those two calls (logits in the plan's workspace) where the fused epilogue does not
// apply: more than 4 classes, vote mode, or slices too small for the direct head kernel.
extern "C" int vs_unet_forward_to_volume(vs_unet_t* net, const float* params, float* bnstate, const float* x, int n,
                                         void* workspace, void* stream, const vs_dirmap* m, int s0, int mode, int direction,
                                         uint8_t* labels, uint16_t* probs, uint32_t* keys, uint8_t* votes, int64_t nvox) {
    VS_REQUIRE(net && m, "unet_forward_to_volume: null pointer");
    VS_REQUIRE(m->hp == net->h && m->wp == net->w, "unet_forward_to_volume: the plan is %dx%d, the padded slices are %dx%d", net->h, net->w, m->hp, m->wp);
    VS_REQUIRE(direction >= 0 && direction < 16, "unet_forward_to_volume: direction %d out of range", direction);
    VolScatter sc{};
    sc.m = *m; sc.s0 = s0; sc.direction = direction; sc.mode = mode; sc.labels = labels; sc.probs = probs; sc.keys = keys;
    float* lg = reinterpret_cast<float*>((char*)workspace + net->off_logits);
    const bool try_fused = mode == 0 || mode == 1;
    // slices along the volume's contiguous axis: the head stages its keys slice-major in the (otherwise unused) logits
    // buffer and a transposing pass merges them into the volume along that axis
    const bool staged = mode == 1 && (m->ss == 1 || m->ss == -1) && m->sw != 1 && m->sw != -1 && n >= 8;
    if (staged) sc.stage = reinterpret_cast<uint32_t*>(lg);
    const int rc = unet_forward(net, params, bnstate, x, n, 0, lg, workspace, stream, try_fused ? &sc : nullptr);
    if (rc < 0) return rc;
    if (try_fused && rc == VS_OK)                 // the head kernel already wrote the volume entries (or staged the keys)
        return staged ? launch_keys_stage_scatter(sc.stage, n, *m, s0, keys, (hipStream_t)stream) : VS_OK;
    return vs_logits_to_volume(lg, net->classes, m, s0, n, mode, direction, labels, probs, keys, votes, nvox, stream);
}

// ---- backward --------------------------------------------------------------------------------------
extern "C" int vs_unet_backward(vs_unet_t* net, const float* params, const float* x, const float* dlogits, int n,
                                int need_encoder_wgrad, float* grads, void* workspace, void* stream) {
    VS_REQUIRE(net, "unet_backward: null pointer");
    return unet_backward_range(net, params, x, dlogits, n, need_encoder_wgrad, grads, workspace, stream, 0, (int)net->units.size(), nullptr);
}

// Backward of the units [unit_lo, unit_hi) only (processed from unit_hi-1 down to unit_lo).  Calling it for consecutive
// ranges from the top of the network down is identical to one vs_unet_backward call; when it returns, every gradient of
// the range is ordered on the caller's stream (the side stream is joined), so a data-parallel caller can all-reduce that
// slice of the flat gradient buffer while the next range runs.
extern "C" int vs_unet_backward_range(vs_unet_t* net, const float* params, const float* x, const float* dlogits, int n,
                                      int need_encoder_wgrad, float* grads, void* workspace, void* stream, int unit_lo,
                                      int unit_hi) {
    VS_REQUIRE(net && unit_lo >= 0 && unit_lo < unit_hi && unit_hi <= (int)net->units.size(), "unet_backward_range: bad unit range");
    return unet_backward_range(net, params, x, dlogits, n, need_encoder_wgrad, grads, workspace, stream, unit_lo, unit_hi, nullptr);
}

extern "C" int vs_unet_backward_adamw(vs_unet_t* net, const float* x, const float* dlogits, int n, int need_encoder_wgrad,
                                      float* grads, void* workspace, void* stream, const vs_adamw_args* opt) {
    VS_REQUIRE(net && opt && opt->params && opt->exp_avg && opt->exp_avg_sq && opt->step >= 1, "unet_backward_adamw: bad optimiser arguments");
    return unet_backward_range(net, opt->params, x, dlogits, n, need_encoder_wgrad, grads, workspace, stream, 0,
                               (int)net->units.size(), opt);
}

// One stream's share of vs_unet_backward_adamw for the units [unit_lo, unit_hi) (see ROLE_* above): role 1 = the caller's-stream
// kernels (BatchNorm backward, data gradients), role 2 = weight gradients + AdamW + next-forward weight copies, each
// enqueued in order on `stream`; the caller orders role 2 of a range behind role 1 of the same range.  No weight-set flip.
extern "C" int vs_unet_backward_adamw_part(vs_unet_t* net, const float* x, const float* dlogits, int n, int need_encoder_wgrad,
                                           float* grads, void* workspace, void* stream, const vs_adamw_args* opt, int unit_lo,
                                           int unit_hi, int role) {
    VS_REQUIRE(net && opt && opt->params && opt->exp_avg && opt->exp_avg_sq && opt->step >= 1, "unet_backward_adamw_part: bad optimiser arguments");
    VS_REQUIRE(unit_lo >= 0 && unit_lo < unit_hi && unit_hi <= (int)net->units.size(), "unet_backward_adamw_part: bad unit range");
    VS_REQUIRE(role == ROLE_MAIN || role == ROLE_SIDE, "unet_backward_adamw_part: role must be 1 (caller's stream) or 2 (weight gradients)");
    return unet_backward_range(net, opt->params, x, dlogits, n, need_encoder_wgrad, grads, workspace, stream, unit_lo, unit_hi, opt, role);
}

// Data-parallel form of the split roles: the same two shares WITHOUT the optimiser (role 2 = weight gradients only, written to
// `grads`), so the caller can all-reduce a range's gradient slice before vs_unet_adamw_range updates it.
extern "C" int vs_unet_backward_part(vs_unet_t* net, const float* params, const float* x, const float* dlogits, int n,
                                     int need_encoder_wgrad, float* grads, void* workspace, void* stream, int unit_lo,
                                     int unit_hi, int role) {
    VS_REQUIRE(net && unit_lo >= 0 && unit_lo < unit_hi && unit_hi <= (int)net->units.size(), "unet_backward_part: bad unit range");
    VS_REQUIRE(role == ROLE_MAIN || role == ROLE_SIDE, "unet_backward_part: role must be 1 (caller's stream) or 2 (weight gradients)");
    return unet_backward_range(net, params, x, dlogits, n, need_encoder_wgrad, grads, workspace, stream, unit_lo, unit_hi, nullptr, role);
}

// AdamW over the parameters of the units [unit_lo, unit_hi) from `grads` (e.g. an all-reduced slice) plus the weight copies
// of those units for the next forward, in order on `stream`; no weight-set flip (vs_unet_flip_weight_set once every range
// of the step is queued).  The optimiser step of vs_unet_backward_adamw, cut loose from the backward pass.
extern "C" int vs_unet_adamw_range(vs_unet_t* net, int need_encoder_wgrad, const float* grads, void* workspace, void* stream,
                                   const vs_adamw_args* opt, int unit_lo, int unit_hi) {
    VS_REQUIRE(net && grads && workspace && opt && opt->params && opt->exp_avg && opt->exp_avg_sq && opt->step >= 1,
               "unet_adamw_range: bad arguments");
    VS_REQUIRE(unit_lo >= 0 && unit_lo < unit_hi && unit_hi <= (int)net->units.size(), "unet_adamw_range: bad unit range");
    Ctx c{net, (char*)workspace, opt->params, nullptr, (hipStream_t)stream, net->last_n};
    return update_units(c, unit_lo, unit_hi, need_encoder_wgrad != 0, grads, *opt, (hipStream_t)stream);
}

// ---- cross-rank BatchNorm statistics ---------------------------------------------------------------------
// SyncBatchNorm for data-parallel training: `hook` sums device values in place over the ranks (stream-ordered; see BnSync in common.h),
// `world` ranks contribute equal shares of the global batch.  With it every BatchNorm of a training forward normalises with the
// statistics of the GLOBAL batch (the unit's fixed-point sums are added over the ranks before the normalisation sweep: integer
// sums, so every rank forms the same bits and the result equals a single process running the whole batch), and the backward pass
// sums (sum dy, sum dy xhat) over the ranks for dx.  hook = null: back to per-rank statistics.  Built for bf16 plans whose
// BatchNorms all sit behind bias-free convolutions or the ResNet stem (U-Net / U-Net++ / FPN over the ResNet / ResNeXt encoders -
// BASELINE configs[3]); other plans are refused here.  Replaces nothing in the reference (it is single-GPU: one loader, one
// BatchNorm batch - data/dataloaders.py:42-49); it is what makes N ranks reproduce that single batch.
extern "C" int vs_unet_set_stats_hook(vs_unet_t* net, vs_stats_hook_fn hook, void* user, int world) {
    VS_REQUIRE(net && world >= 1, "vs_unet_set_stats_hook: bad arguments");
    if (hook) {
        VS_REQUIRE(net->dtype == VS_BF16, "vs_unet_set_stats_hook: cross-rank BatchNorm statistics are built for bf16 plans (fixed-point statistics bins)");
        for (const Unit& u : net->units) {
            const bool ok_bn = (u.kind == U_CONV && (u.bn_idx < 0 || (u.bias_idx < 0 && u.off_bins))) || (u.kind == U_STEM && u.off_bins) ||
                               (u.kind != U_CONV && u.kind != U_STEM && u.kind != U_BN && u.kind != U_CONVT && u.kind != U_FPA);
            VS_REQUIRE(ok_bn, "vs_unet_set_stats_hook: this network has BatchNorm layers outside bias-free convolution units (transposed convolutions, "
                              "standalone norms, biased convolutions, the FPA block): SyncBatchNorm is not built for them");
        }
    }
    net->stats_hook = hook; net->stats_user = user; net->stats_world = hook ? world : 1;
    return VS_OK;
}

// Which units' outputs a bf16 training forward at batch n would NOT materialise (normalise-on-load, see nl_consumer): flags[i] = 1
// for such a unit i.  Host logic only - nothing is launched (tests, tools).  Returns the number of units.
extern "C" int vs_unet_nl_plan(vs_unet_t* net, int n, int* flags, int cap) {
    VS_REQUIRE(net && flags && n >= 1 && n <= net->max_batch, "vs_unet_nl_plan: bad arguments");
    Ctx c{net, reinterpret_cast<char*>(uintptr_t(1) << 20), nullptr, nullptr, nullptr, n};   // (addresses are never dereferenced)
    for (int i = 0; i < (int)net->units.size() && i < cap; ++i) flags[i] = nl_consumer(c, i) >= 0;
    return (int)net->units.size();
}
