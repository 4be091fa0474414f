// The network plan: the data model that unet_plan.hip builds and lays out and that unet.hip reads when it enqueues a pass.
//
// A plan is a flat list of units over activations and the tensors of the state dict, with every activation, gradient and scratch
// buffer laid out once in a caller-owned workspace (struct vs_unet).  unet_plan.hip constructs, lays out and describes plans and
// launches nothing; unet.hip enqueues the passes and moves no plan.  The internal types live in namespace unet (mesh.hip has a Layout of
// its own); struct vs_unet is the C handle type and stays global.
#pragma once
#include <string>
#include <vector>

#include "common.h"

namespace unet {

struct TensorInfo {
    std::string name;
    int64_t shape[4];
    int ndim, kind;
    int64_t offset;
};
inline int64_t tensor_elems(const TensorInfo& t) {
    int64_t n = 1;
    for (int d = 0; d < t.ndim; ++d) n *= t.shape[d];
    return n;
}

// What each kind computes is stated where its forward and its backward are enqueued ("the units" in unet.hip).
enum UnitKind { U_STEM, U_POOL, U_CONV, U_HEAD, U_CONCAT, U_CONVT, U_ADD, U_UPADD, U_BILINEAR, U_DROPOUT, U_DWCONV, U_GAP, U_BCAST, U_DROPOUT_E,
                U_PAB, U_SE, U_CGATE, U_SIGMOID, U_BN, U_DWCONV2, U_DROPADD, U_FOLD2, U_RSOFTMAX, U_RADIXSUM, U_AVGPOOL, U_UP2, U_FPA };

struct Act {  // one activation tensor (per-sample element count = c*h*w)
    int c, h, w;
    bool has_z;
    size_t off_a = 0, off_z = 0, off_da = 0, off_dz = 0;
};

// rows of fixed-point statistics bins of a unit (ConvParams::stats_bins): enough rows that an address takes ~16 - 32 atomic adds per
// launch (16 rows for the tile kernels' 256 - 512 tiles; 256 for the <= 16-channel layers, whose direct kernel adds once per WAVE)
static inline int stat_bins_rows(int cout) { return cout <= 16 ? 256 : 16; }
static inline size_t unit_bins_bytes(int cout) { return (size_t)stat_bins_rows(cout) * 2 * cout * sizeof(unsigned long long); }
constexpr size_t kTicketBytes = 128;   // behind a unit's bins: the ticket counter of ConvParams::fin_ticket (cleared with the bins)

struct Unit {
    UnitKind kind;
    int src0 = -1, src1 = -1, up0 = 0;  // input activation ids
    int cin0 = 0, cin1 = 0, cout = 0, k = 3, stride = 1, pad = 1;
    int hin = 0, win = 0, hout = 0, wout = 0;  // virtual input / output spatial dims
    int w_idx = -1, bn_idx = -1, bias_idx = -1;  // indices into the tensor table (bn_idx -> gamma)
    int out = -1;   // output activation id
    int res = -1;   // residual activation id
    int relu = 1;
    int gn_idx = -1, gn_groups = 0;   // U_CONV followed by nn.GroupNorm(gn_groups, cout) + ReLU instead of BatchNorm (gamma at gn_idx)
    size_t off_gn = 0;                // its statistics [n][groups][2] fp32
    float bn_eps = 1e-5f, bn_mom = 0.1f;   // U_BN
    float drop_p = 0.f; int salt = 0;      // U_DROPADD: drop-connect rate, block index (separates the blocks' draws)
    int bcast = 0;                         // U_DWCONV2 on the single-channel network input
    int g2 = 0;                            // U_CONV: cin -> cout = 2 cin in TWO groups (ResNeSt's radix-2 split-attention 3x3); weights [cout][taps][cin / 2],
                                           // the compute copies dense with the other group's half zero (optim.hip: two_groups)
    bool aux_frozen = false;               // the unit's BatchNorm / bias tensors also match the freeze predicate ("encoder" and "conv" in the name)
    float pool_w = 0.f;                    // U_AVGPOOL: the constant tap (1 / 9 or 1 / 4)
    int dil = 1;    // dilation of a stride-1 3x3 convolution (2: smp's replace_strides_with_dilation; any for U_DWCONV)
    int factor = 2; // U_BILINEAR: integer scale factor
    int colr = 0;   // U_CONV: a 3x3 convolution with dilation = padding = colr (DeepLabV3's dense ASPP rates 12 / 24 / 36), run as the
                    // 1x1 convolution over the 9 * cin channels of its input's column form (vs_dilated_im2col)
    size_t off_xs = 0;   // that column form (kept for the weight gradient)
    int cg = 0;     // grouped convolution (ResNeXt): channels per group, cin0 == cout; 0 = dense.  Weights [cout][k*k][cg]; the
                    // compute copies are block-expanded to 32-channel super-groups (vs_weights_prepare_grouped)
    bool frozen_candidate = false;  // "encoder" in name and "conv" in name (vol_seg_2d_trainer.py:102-108)
    size_t off_wc = 0, off_wt = 0, off_bn = 0;  // workspace offsets (bytes): weight copies, 4*C floats of BN constants
    size_t off_bins = 0;                         // stat_bins_rows(cout) rows of fixed-point statistics bins ([row][2][cout] 64-bit), training plans
    size_t off_wc2 = 0, off_wt2 = 0;             // second set of weight copies (training workspaces): see vs_unet::wset
    std::vector<int> tens;                       // U_FPA: parameter tensor indices
    size_t off_fpa_pool = 0, off_fpa_arena = 0, off_fpa_plane = 0;   // U_FPA: pooled input, pyramid arena (fp32), attention plane (fp32)
    std::vector<int> members;                    // U_CONCAT: the activations whose channels `out` strings together, in order
};

struct Layout {
    std::vector<TensorInfo> tensors;
    int64_t n_params = 0, n_bnstate = 0;
};

}  // namespace unet

struct vs_unet {
    int dtype, classes, max_batch, h, w;
    int topology = 0;   // smp's decoder: 0 Unet, 1 UnetPlusPlus, 2 Linknet, 3 FPN, 4 DeepLabV3Plus, 5 DeepLabV3, 6 MAnet, 7 PAN
    int encoder = 34;   // smp's encoder_name: 18 / 34 / 50 = resnet18 / 34 / 50, 51 = resnext50_32x4d, 103 / 104 = efficientnet-b3 / b4,
                        // 150 = timm-resnest50d, 201 = timm-resnest101e (the pairs that are built: check_network_code in unet_plan.hip)
    unet::Layout layout;
    std::vector<unet::Act> acts;
    std::vector<unet::Unit> units;
    size_t esz;
    // workspace regions (bytes)
    size_t off_bins0 = 0, bins_bytes = 0;        // all units' statistics bins, contiguous: zeroed by ONE launch per training forward
    size_t off_bnws = 0, bnws_bytes = 0, off_wgws = 0, wgws_bytes = 0, off_headdw = 0, off_headpart = 0, off_dyh = 0, off_dup = 0,
           off_zs = 0, off_idx = 0;
    size_t ws_eval = 0, ws_train = 0, off_logits = 0;
    size_t off_bncnt = 0;                        // reserved, unused: 256 bytes that keep every later offset (and the pinned plans) where it is
    int last_n = 0;
    std::vector<char> group_first;  // optimiser groups of the fused backward (see unet_backward_range)
    std::vector<int> producer, first_consumer;   // per activation: unit that outputs it / lowest-index unit that reads it
    std::vector<int> bwd_stat_rows;              // per activation: partial rows left by the dgrad that completed its gradient
    std::vector<int> sole_consumer;              // per activation: the ONE unit that reads it (-1: none / several readers)
    // SyncBatchNorm under data parallelism (vs_unet_set_stats_hook): the statistics of every BatchNorm are summed over the ranks
    vs_stats_hook_fn stats_hook = nullptr; void* stats_user = nullptr; int stats_world = 1;
    size_t off_syncsc = 0;                       // 2 * cmax floats: the summed copies of a unit's (dbeta, dgamma) for the backward apply
    std::vector<char> nl_act;                    // per activation, set by the last training forward: it was never materialised - its one
                                                 // consumer normalises the producer's pre-norm output z while loading it (ConvParams::nl_*)
    size_t off_gnz = 0, off_gnws = 0, gnws_bytes = 0, off_dropmask = 0, off_lsmall = 0, off_dlsmall = 0;   // smp.FPN (see plan_workspace)
    int head_up = 1;                   // the head works at 1 / head_up resolution, nn.UpsamplingBilinear2d(head_up) follows (FPN: 4)
    uint32_t rng_seed = 0; const int64_t* rng_counter = nullptr;   // Dropout2d draws (vs_unet_set_rng)
    size_t off_pab = 0, pab_bytes = 0; // scratch of the PAB attention (vs_pab_scratch_bytes)
    size_t off_sews = 0;               // scratch of the squeeze-excitation gates' backward pass (vs_se_gate_scratch_floats)
    size_t off_gapws = 0, gapws_bytes = 0;   // split partial sums of the average pools / gate gradients (vs_sample_rowsum_ws)
    size_t off_avgw9 = 0, off_avgw4 = 0; int avgw_c = 0;   // constant taps of U_AVGPOOL: [c][9] of 1 / 9 and [c][4] of 1 / 4
    size_t off_ys = 0;                 // scratch: the column form of a large-rate convolution's input gradient
    size_t off_ct = 0, off_ctdw = 0, ctdw_bytes = 0;   // transposed convolutions: un-shuffled output; dense 3x3 weight gradient
    int wset = 0;  // which set of weight copies the forward / backward read; the fused optimiser step fills the other and flips
    std::vector<char> written;  // per activation: has its gradient buffer been written in the current backward pass
    // backward runs the weight-gradient kernels on an internal side stream, forked from / joined to the caller's stream
    static constexpr int kSide = 2;
    hipStream_t side[kSide] = {nullptr, nullptr};
    std::vector<hipEvent_t> fork_events;
    hipEvent_t join_event[kSide] = {nullptr, nullptr};
    ~vs_unet() {
        for (auto e : fork_events) (void)hipEventDestroy(e);
        for (int i = 0; i < kSide; ++i)
            if (join_event[i]) (void)hipEventDestroy(join_event[i]);   // (the side streams belong to the process-wide pool in unet.hip)
    }
};

namespace unet {

// bytes of a convolution's two prepared weight copies: wc [cout][taps][cin] in the compute dtype and wt, its flipped / transposed twin
// for the data gradient (grouped layers: 32-channel super-groups; the head's wt pads to 16 output channels; a transposed convolution
// has the copies of its equivalent 3x3 convolution onto 4 * cout channels).  The same for both weight sets.
struct WeightCopyBytes { size_t wc, wt; };
inline WeightCopyBytes weight_copy_bytes(const Unit& u, size_t esz) {
    if (u.kind == U_CONVT) return {(size_t)4 * u.cout * 9 * u.cin0 * esz, (size_t)u.cin0 * 9 * 4 * u.cout * esz};
    const size_t taps = (size_t)u.k * u.k, cin = (size_t)u.cin0 + u.cin1;
    const size_t cout_pad = u.kind == U_HEAD ? 16 : (size_t)u.cout;
    return {(size_t)u.cout * taps * (u.cg ? 32 : cin) * esz, cin * taps * (u.cg ? 32 : cout_pad) * esz};
}
// the units with fixed-point statistics bins (ConvParams::stats_bins): bias-free convolution + BatchNorm, and the ResNet stem
inline bool has_stat_bins(const Unit& u) { return (u.kind == U_CONV && u.bn_idx >= 0 && u.bias_idx < 0) || (u.kind == U_STEM && u.cout == 64); }

// the forward reads a prepared copy of the unit's weight, not the fp32 master: low precision, or a layout that only the copy has
inline bool has_weight_copy(const vs_unet* net, const Unit& u) { return net->dtype != VS_F32 || u.cg || u.g2; }

// the standalone BatchNorm unit (U_BN) right behind unit ui that reads its output - EfficientNet's norms, which ride in the epilogue of
// the convolution in front of them where that can be done - or null
inline const Unit* bn_behind(const vs_unet* net, int ui) {
    if (ui + 1 >= (int)net->units.size()) return nullptr;
    const Unit& v = net->units[ui + 1];
    return (v.kind == U_BN && v.src0 == net->units[ui].out) ? &v : nullptr;
}

// ---- what unet.hip calls in unet_plan.hip ----
// producer / consumer maps of the activation graph (built once)
void ensure_graph_maps(vs_unet* net);

}  // namespace unet
