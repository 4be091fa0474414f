// Network plans: everything that constructs, lays out or describes one, and nothing that launches.
//
// build_plan() strings the units of one of the 56 networks together - smp's Unet / UnetPlusPlus / Linknet / FPN / DeepLabV3Plus /
// DeepLabV3 / MAnet / PAN over the resnet18 / 34 / 50, resnext50_32x4d, efficientnet-b3 / b4 and timm-resnest50d / 101e encoders
// with one input channel (reference construction: volume_segmantics/model/model_2d.py:15-16; topologies: SURVEY.md section 8a) -
// and registers the tensors of its state dict; plan_workspace() gives every weight copy, activation, gradient and scratch buffer its
// offset in the caller-owned workspace.  Behind them the C entry points that create, destroy and describe a plan: the parameter table,
// the workspace size, the unit and mask queries and the plan dump.  The passes over a plan are enqueued by unet.hip.
#include <cmath>
#include <cstdlib>
#include <string>
#include <vector>

#include "common.h"
#include "unet_plan.h"

using namespace unet;

namespace {

void add_tensor(Layout& L, const std::string& name, std::initializer_list<int64_t> shape, int kind) {
    TensorInfo t;
    t.name = name;
    t.ndim = (int)shape.size();
    int64_t numel = 1;
    int i = 0;
    for (auto s : shape) { t.shape[i++] = s; numel *= s; }
    for (; i < 4; ++i) t.shape[i] = 1;
    t.kind = kind;
    if (kind <= 3) { t.offset = L.n_params; L.n_params += numel; }
    else { t.offset = L.n_bnstate; L.n_bnstate += numel; }
    L.tensors.push_back(t);
}

// returns index of gamma
int add_bn(Layout& L, const std::string& prefix, int c) {
    const int idx = (int)L.tensors.size();
    add_tensor(L, prefix + ".weight", {c}, 1);
    add_tensor(L, prefix + ".bias", {c}, 2);
    add_tensor(L, prefix + ".running_mean", {c}, 4);
    add_tensor(L, prefix + ".running_var", {c}, 5);
    return idx;
}

// ---- plan construction ------------------------------------------------------------------------------------------------------------
// A plan is three ordered lists: the tensors of the state dict (Layout), the activations and the units.  Tensor indices fix the
// state-dict layout, activation ids fix every workspace offset, the unit order is the forward order.  The three orders are independent
// of one another, and each is part of a construction: WHEN a constructor registers its tensors, allocates its output and emits its unit
// is stated where it differs from "all three at once" (tests/test_host_logic.py test_every_network_plan_is_the_recorded_one pins them).
struct Builder {
    vs_unet* net;
    Layout& L;
    std::vector<Act>& A;
    std::vector<Unit>& U;
    explicit Builder(vs_unet* n) : net(n), L(n->layout), A(n->acts), U(n->units) {}

    int act(int c, int h, int w, bool has_z) {
        Act a; a.c = c; a.h = h; a.w = w; a.has_z = has_z;
        A.push_back(a);
        return (int)A.size() - 1;
    }
    int tensor(const std::string& name, std::initializer_list<int64_t> shape, int kind) {
        add_tensor(L, name, shape, kind);
        return (int)L.tensors.size() - 1;
    }
    int weight(const std::string& name, std::initializer_list<int64_t> shape) { return tensor(name, shape, 0); }
    int bias(const std::string& name, int c) { return tensor(name, {c}, 3); }
    int bn(const std::string& prefix, int c) { return add_bn(L, prefix, c); }   // index of gamma

    // a convolution described - k x k, padding k / 2, h x w -> h / stride x w / stride, ReLU - with nothing registered or allocated yet
    static Unit conv(int src, int cin, int cout, int k, int stride, int h, int w) {
        Unit u; u.kind = U_CONV; u.src0 = src; u.cin0 = cin; u.cout = cout; u.k = k; u.pad = k / 2; u.stride = stride;
        u.hin = h; u.win = w; u.hout = h / stride; u.wout = w / stride;
        return u;
    }
    // cin_w: input channels of one filter where that is not cin0 (grouped convolutions)
    void attach_weight(Unit& u, const std::string& name, int cin_w = 0) { u.w_idx = weight(name, {u.cout, cin_w ? cin_w : u.cin0, u.k, u.k}); }
    void attach_bias(Unit& u, const std::string& name) { u.bias_idx = bias(name, u.cout); }
    void attach_bn(Unit& u, const std::string& prefix) { u.bn_idx = bn(prefix, u.cout); }
    void attach_gn(Unit& u, const std::string& prefix, int groups) {
        u.gn_groups = groups;
        u.gn_idx = tensor(prefix + ".weight", {u.cout}, 1);
        tensor(prefix + ".bias", {u.cout}, 2);
    }
    int emit(const Unit& u) { U.push_back(u); return u.out; }

    // THE convolution constructor: described as conv(), its tensors registered in state-dict order - weight, bias (name not empty),
    // BatchNorm (prefix not empty) - and its output ALLOCATED, with a pre-norm tensor z where a norm follows.  The caller sets what
    // differs (relu, freeze flags, dilation ..) and emits it - at once, or after other units whose activations then get higher ids.
    Unit conv_unit(const std::string& wname, const std::string& bias_name, const std::string& bn_prefix, int src, int cin, int cout, int k,
                   int stride, int h, int w, int cin_w = 0) {
        Unit u = conv(src, cin, cout, k, stride, h, w);
        attach_weight(u, wname, cin_w);
        if (!bias_name.empty()) attach_bias(u, bias_name);
        if (!bn_prefix.empty()) attach_bn(u, bn_prefix);
        u.out = act(cout, u.hout, u.wout, !bn_prefix.empty());
        return u;
    }
    // A unit without parameters, emitted: kind, sources, channels, and the sizes its site sets - many leave hin / win at 0, and the
    // plan keeps that.  relu = 0 (U_POOL alone keeps the struct's default of 1: see its sites).  The reference is good until the next emit.
    Unit& op(UnitKind kind, int src0, int src1, int c, int hin, int win, int hout, int wout) {
        Unit u; u.kind = kind; u.src0 = src0; u.src1 = src1; u.cout = c; u.hin = hin; u.win = win; u.hout = hout; u.wout = wout; u.relu = 0;
        u.out = act(c, hout, wout, false);
        U.push_back(u);
        return U.back();
    }
    int gap(int src, int c, int h, int w) { return op(U_GAP, src, -1, c, h, w, 1, 1).out; }   // nn.AdaptiveAvgPool2d(1)
    int concat(const std::vector<int>& members, int c, int h, int w) {
        Unit& u = op(U_CONCAT, -1, -1, c, 0, 0, h, w);
        u.members = members;
        return u.out;
    }
    int maxpool(int src, int c, int h, int w) {   // nn.MaxPool2d(3, 2, 1)
        Unit& u = op(U_POOL, src, -1, c, h, w, h / 2, w / 2);
        u.relu = 1;
        return u.out;
    }
    // standalone BatchNorm2d + activation (0 none / 1 ReLU / 2 swish), emitted
    Unit& bn_unit(const std::string& prefix, int src, int c, int h, int w, int activation) {
        Unit u; u.kind = U_BN; u.src0 = src; u.cin0 = c; u.cout = c; u.hin = u.hout = h; u.win = u.wout = w; u.relu = activation;
        u.bn_idx = bn(prefix, c); u.out = act(c, h, w, false);
        U.push_back(u);
        return U.back();
    }
    // depthwise k x k convolution with `pad` zero rows / columns in front, no norm, emitted; bcast: on the single-channel network input
    int dwconv2(const std::string& wname, int src, int c, int k, int stride, int pad, int dil, int h, int w, int bcast) {
        Unit u; u.kind = U_DWCONV2; u.src0 = src; u.cin0 = bcast ? 1 : c; u.cout = c; u.k = k; u.stride = stride; u.dil = dil; u.pad = pad;
        u.hin = h; u.win = w; u.hout = h / stride; u.wout = w / stride; u.bcast = bcast; u.relu = 0; u.frozen_candidate = true;
        u.w_idx = weight(wname, {c, 1, k, k});
        u.out = act(c, u.hout, u.wout, false);
        return emit(u);
    }
    // a squeeze-excitation gate: its four tensors W1, b1, W2, b2 (returns the index of W1), and - not always right behind them - the
    // unit on the pooled feature `src`; `activation` is what the site puts into Unit::relu (EfficientNet 2 = swish, MA-Net 0)
    int se_tensors(const std::string& reduce, const std::string& expand, int c, int hidden) {
        const int w = weight(reduce + ".weight", {hidden, c, 1, 1}); bias(reduce + ".bias", hidden);
        weight(expand + ".weight", {c, hidden, 1, 1}); bias(expand + ".bias", c);
        return w;
    }
    int se(int src, int c, int hidden, int widx, int activation) {
        Unit& u = op(U_SE, src, -1, c, 0, 0, 1, 1);
        u.cin0 = c; u.cin1 = hidden; u.w_idx = widx; u.relu = activation;
        return u.out;
    }
};

// activations / channels of the encoder features the decoder taps: [1] the stem at stride 2 .. [5] the deepest
struct Features { int feat[6] = {-1, -1, -1, -1, -1, -1}, featc[6] = {0, 64, 0, 0, 0, 0}; };
struct HeadInput { int act, c, k, up; };   // what a decoder hands to the segmentation head: its input, the head's kernel size, the upsampling behind it

// dilation of encoder stage `stage` (0 .. 3 = layer1 .. layer4) under the dilating decoders (smp's replace_strides_with_dilation):
// DeepLabV3+ (output stride 16) and PAN (encoder_dilation): the last stage with dilation 2; DeepLabV3 (output stride 8): stage 2 with 2, stage 3 with 4
int stage_dilation(int topology, int stage) {
    if (topology == 4 || topology == 7) return stage == 3 ? 2 : 1;
    if (topology == 5) return stage == 2 ? 2 : (stage == 3 ? 4 : 1);
    return 1;
}

Features encoder_efficientnet(Builder& B) {
    // smp's EfficientNetEncoder (encoders/efficientnet.py) over efficientnet-pytorch 0.6.3's EfficientNet-b3 / b4: stem 3x3 / 2 + BN +
    // swish; MBConv blocks = [expand 1x1 + BN + swish] depthwise k x k + BN + swish, squeeze-excitation (hidden = max(1, input
    // filters / 4), swish), project 1x1 + BN, drop_connect(0.2 * i / blocks) + skip when the shape is kept; BatchNorm2d(momentum 0.01,
    // eps 1e-3); Conv2dStaticSamePadding at the (even) nominal image size: (0, 1) for k = 3 and (1, 2) for k = 5 at stride 2.
    // _conv_head / _bn1 stay in the state dict and are never run.  Registration order = execution order.
    const vs_unet* net = B.net;
    const int H = net->h, W = net->w;
    Features f;
    const bool b4 = net->encoder == 104;
    const double width = b4 ? 1.4 : 1.2, depth = b4 ? 1.8 : 1.4;
    auto round_filters = [&](int c) { const double x = c * width; int nw = std::max(8, (int)(x + 4) / 8 * 8); if (nw < 0.9 * x) nw += 8; return nw; };
    auto round_repeats = [&](int r) { return (int)std::ceil(depth * r); };
    static const int base[7][6] = {{1, 3, 1, 1, 32, 16}, {2, 3, 2, 6, 16, 24}, {2, 5, 2, 6, 24, 40}, {3, 3, 2, 6, 40, 80}, {3, 5, 1, 6, 80, 112},
                                   {4, 5, 2, 6, 112, 192}, {1, 3, 1, 6, 192, 320}};
    static const int ends_b3[4] = {5, 8, 18, 26}, ends_b4[4] = {6, 10, 22, 32};
    const int* ends = b4 ? ends_b4 : ends_b3;
    auto bn_unit = [&](const std::string& name, int src, int cch, int hh, int ww, int act) {
        Unit& u = B.bn_unit(name, src, cch, hh, ww, act);
        u.bn_eps = 1e-3f; u.bn_mom = 0.01f;
        return u.out;
    };
    auto pw_conv = [&](const std::string& name, int src, int cin, int cout, int hh, int ww) {    // 1x1, no bias, no norm of its own
        Unit u = B.conv_unit(name, "", "", src, cin, cout, 1, 1, hh, ww);
        u.relu = 0; u.frozen_candidate = true;
        return B.emit(u);
    };
    auto dw_conv = [&](const std::string& name, int src, int cch, int k, int st, int hh, int ww, int bcast, int dil = 1) {
        const int pad = dil > 1 ? (k / 2) * dil : (st == 2 ? (k == 3 ? 0 : 1) : k / 2);
        return B.dwconv2(name, src, cch, k, st, pad, dil, hh, ww, bcast);
    };
    const int stem_c = round_filters(32);
    int cur = dw_conv("encoder._conv_stem.weight", -1, stem_c, 3, 2, H, W, 1);
    cur = bn_unit("encoder._bn0", cur, stem_c, H / 2, W / 2, 2);
    f.feat[1] = cur; f.featc[1] = stem_c;
    int ch = H / 2, cw = W / 2, inpl = 64;
    int nblocks = 0;
    for (auto& b : base) nblocks += round_repeats(b[0]);
    int bi = 0, stage = 0;
    for (auto& b : base) {
        const int k = b[1], e = b[3], o = round_filters(b[5]);
        for (int j = 0; j < round_repeats(b[0]); ++j, ++bi) {
            // DeepLabV3+ (output stride 16): smp's replace_strides_with_dilation on the last stage (blocks[ends[2]:]) - every
            // convolution stride 1, dilation 2, padding (k / 2) * 2, the static padding dropped ("Kostyl for EfficientNet")
            // DeepLabV3 (output stride 8): stages 4 and 5 (blocks[ends[1]:ends[2]], blocks[ends[2]:]) with dilation 2 and 4
            // PAN (encoder_dilation): the last stage with dilation 2, as DeepLabV3+
            const int stage_dil = stage_dilation(net->topology, bi >= ends[2] ? 3 : (bi >= ends[1] ? 2 : 1));
            const bool dilated = stage_dil > 1;
            const int st = (j == 0 && !dilated) ? b[2] : 1, inp = j == 0 ? round_filters(b[4]) : o, oup = inp * e;
            const std::string pre = "encoder._blocks." + std::to_string(bi);
            const int x_in = cur;
            int t = cur;
            if (e != 1) {
                t = pw_conv(pre + "._expand_conv.weight", t, inp, oup, ch, cw);
                t = bn_unit(pre + "._bn0", t, oup, ch, cw, 2);
            }
            t = dw_conv(pre + "._depthwise_conv.weight", t, oup, k, st, ch, cw, 0, stage_dil);
            const int oh = ch / st, ow = cw / st;
            t = bn_unit(pre + "._bn1", t, oup, oh, ow, 2);
            const int R = std::max(1, inp / 4);
            const int pooled = B.gap(t, oup, oh, ow);
            const int gate = B.se(pooled, oup, R, B.se_tensors(pre + "._se_reduce", pre + "._se_expand", oup, R), 2);
            const int gated = B.op(U_CGATE, t, gate, oup, 0, 0, oh, ow).out;
            t = pw_conv(pre + "._project_conv.weight", gated, oup, o, oh, ow);
            t = bn_unit(pre + "._bn2", t, o, oh, ow, 0);
            if (st == 1 && inp == o) {
                Unit& da = B.op(U_DROPADD, t, x_in, o, oh, ow, oh, ow);
                da.drop_p = 0.2f * (float)bi / (float)nblocks; da.salt = bi;
                t = da.out;
            }
            cur = t; ch = oh; cw = ow; inpl = o;
            if (stage < 4 && bi + 1 == ends[stage]) { f.feat[stage + 2] = cur; f.featc[stage + 2] = o; ++stage; }
        }
    }
    B.weight("encoder._conv_head.weight", {round_filters(1280), inpl, 1, 1});     // registered by efficientnet-pytorch, never run
    B.bn("encoder._bn1", round_filters(1280));
    return f;
}

Features encoder_resnest(Builder& B) {
    // smp's timm-resnest50d / timm-resnest101e (timm 0.4.12 ResNet(ResNestBottleneck, stem_type 'deep', avg_down, radix 2, avd)):
    // deep stem conv1 = [3x3 / 2 (1 -> sw) BN ReLU, 3x3 (sw -> sw) BN ReLU, 3x3 (sw -> 2 sw)], bn1, ReLU, MaxPool(3, 2, 1); blocks = conv1 1x1 +
    // bn1 + ReLU, conv2 = SplitAttnConv2d (3x3 onto 2 C channels in two groups + bn0 + ReLU; the splits summed and average-pooled;
    // fc1 (bias) + bn1 + ReLU; fc2 (bias); RadixSoftmax; the attention-weighted sum of the splits), avd_last = AvgPool2d(3, 2, 1) in
    // the stride-2 blocks, conv3 1x1 + bn3 (+ shortcut, ReLU); shortcut = [AvgPool2d(2, 2)] + 1x1 + BN.  The reference's freeze
    // predicate ("encoder" and "conv" in the name) also takes conv2.bn0 / conv2.fc1 / conv2.bn1 / conv2.fc2 and the stem's BatchNorms.
    const vs_unet* net = B.net;
    const int H = net->h, W = net->w;
    Features f;
    const bool e101 = net->encoder == 201;
    const int sw = e101 ? 64 : 32;
    const int blocks_n[4] = {3, 4, e101 ? 23 : 6, 3};
    // (described, not emitted: conv3 is described - tensors registered, output allocated - BEFORE the shortcut that runs ahead of it)
    auto conv_bn = [&](const std::string& wname, const std::string& bias, const std::string& bnname, int src, int cin, int cout, int k, int hh, int ww,
                       int relu, bool frozen, bool aux_frozen, int two_groups = 0) {
        Unit u = B.conv_unit(wname, bias, bnname, src, cin, cout, k, 1, hh, ww, two_groups ? cin / 2 : 0);
        u.g2 = two_groups; u.relu = relu; u.frozen_candidate = frozen; u.aux_frozen = aux_frozen;
        return u;
    };
    auto avgpool = [&](int src, int c, int k, int pad, int hh, int ww) {
        Unit& ap = B.op(U_AVGPOOL, src, -1, c, hh, ww, hh / 2, ww / 2);
        ap.k = k; ap.stride = 2; ap.pad = pad; ap.pool_w = 1.f / (float)(k * k);
        return ap.out;
    };
    // deep stem
    int cur = B.dwconv2("encoder.conv1.0.weight", -1, sw, 3, 2, 1, 1, H, W, 1);
    Unit& b = B.bn_unit("encoder.conv1.1", cur, sw, H / 2, W / 2, 1);
    b.aux_frozen = true;
    cur = B.emit(conv_bn("encoder.conv1.3.weight", "", "encoder.conv1.4", b.out, sw, sw, 3, H / 2, W / 2, 1, true, true));
    cur = B.emit(conv_bn("encoder.conv1.6.weight", "", "encoder.bn1", cur, sw, 2 * sw, 3, H / 2, W / 2, 1, true, false));
    f.feat[1] = cur; f.featc[1] = 2 * sw;
    cur = B.maxpool(cur, 2 * sw, H / 2, W / 2);
    int inpl = 2 * sw, ch = H / 4, cw = W / 4;
    const int planes_r[4] = {64, 128, 256, 512};
    for (int l = 0; l < 4; ++l) {
        for (int bidx = 0; bidx < blocks_n[l]; ++bidx) {
            const std::string pre = "encoder.layer" + std::to_string(l + 1) + "." + std::to_string(bidx);
            const int stride = (bidx == 0 && l > 0) ? 2 : 1, C = planes_r[l], outc = 4 * C, hidden = std::max(C * 2 / 4, 32);
            const int oh = ch / stride, ow = cw / stride;
            const int x_in = cur;
            const int u1 = B.emit(conv_bn(pre + ".conv1.weight", "", pre + ".bn1", cur, inpl, C, 1, ch, cw, 1, true, false));
            // (conv2.conv's weight: [2 C][C / 2][3][3])
            const int u2 = B.emit(conv_bn(pre + ".conv2.conv.weight", "", pre + ".conv2.bn0", u1, C, 2 * C, 3, ch, cw, 1, true, true, 1));
            const int pooled = B.gap(u2, 2 * C, ch, cw);
            const int folded = B.op(U_FOLD2, pooled, -1, C, 1, 1, 1, 1).out;
            const int f1 = B.emit(conv_bn(pre + ".conv2.fc1.weight", pre + ".conv2.fc1.bias", pre + ".conv2.bn1", folded, C, hidden, 1, 1, 1, 1, true, true));
            const int f2 = B.emit(conv_bn(pre + ".conv2.fc2.weight", pre + ".conv2.fc2.bias", "", f1, hidden, 2 * C, 1, 1, 1, 0, true, true));
            const int attn = B.op(U_RSOFTMAX, f2, -1, 2 * C, 1, 1, 1, 1).out;
            int t = B.op(U_RADIXSUM, u2, attn, C, ch, cw, ch, cw).out;
            if (stride == 2) t = avgpool(t, C, 3, 1, ch, cw);     // avd_last = nn.AvgPool2d(3, 2, padding=1): the padding zeros count (count_include_pad)
            Unit u3 = conv_bn(pre + ".conv3.weight", "", pre + ".bn3", t, C, outc, 1, oh, ow, 1, true, false);
            if (bidx == 0) {        // downsample_avg: [AvgPool2d(2, 2, ceil_mode, count_include_pad=False)] + 1x1 convolution + BatchNorm
                const int ds = stride == 2 ? avgpool(x_in, inpl, 2, 0, ch, cw) : x_in;
                // state-dict order: conv3, bn3, then downsample.* - the tensors of u3 were registered first (conv_bn above)
                u3.res = B.emit(conv_bn(pre + ".downsample.1.weight", "", pre + ".downsample.2", ds, inpl, outc, 1, oh, ow, 0, false, false));
            } else {
                u3.res = x_in;
            }
            cur = B.emit(u3); inpl = outc; ch = oh; cw = ow;
        }
        f.feat[l + 2] = cur; f.featc[l + 2] = inpl;
    }
    return f;
}

Features encoder_resnet(Builder& B) {
    // torchvision's ResNet behind smp's resnet18 / resnet34 / resnet50 / resnext50_32x4d with a single input channel
    const vs_unet* net = B.net;
    const int H = net->h, W = net->w;
    Features f;
    Unit stem; stem.kind = U_STEM; stem.cout = 64; stem.k = 7; stem.stride = 2; stem.pad = 3;
    stem.hin = H; stem.win = W; stem.hout = H / 2; stem.wout = W / 2; stem.frozen_candidate = true;
    stem.w_idx = B.weight("encoder.conv1.weight", {64, 1, 7, 7});
    B.attach_bn(stem, "encoder.bn1");
    stem.out = B.act(64, H / 2, W / 2, true);
    f.feat[1] = B.emit(stem);
    int cur = B.maxpool(stem.out, 64, H / 2, W / 2), inpl = 64, ch = H / 4, cw = W / 4;
    const int planes[4] = {64, 128, 256, 512};
    const int blocks18[4] = {2, 2, 2, 2}, blocks34[4] = {3, 4, 6, 3};   // resnet50 uses the resnet34 block counts
    const int* blocks = net->encoder == 18 ? blocks18 : blocks34;
    const bool bottleneck = net->encoder == 50 || net->encoder == 51;   // 51 = resnext50_32x4d: Bottleneck with groups = 32,
    const int groups = net->encoder == 51 ? 32 : 1;                     // width_per_group = 4 (torchvision): width = planes * 2
    const int expansion = bottleneck ? 4 : 1;
    for (int l = 0; l < 4; ++l) {
        for (int b = 0; b < blocks[l]; ++b) {
            const std::string pre = "encoder.layer" + std::to_string(l + 1) + "." + std::to_string(b);
            // DeepLabV3+ (output stride 16): smp's replace_strides_with_dilation turns layer4's stride into dilation 2 - every
            // convolution of the stage gets stride 1, and the 3x3 ones dilation 2 / padding 2
            // DeepLabV3 (output stride 8): layer3 with dilation 2, layer4 with dilation 4
            // PAN (encoder_dilation=True): layer4 with dilation 2, as DeepLabV3+
            const int stage_dil = stage_dilation(net->topology, l);
            const bool dilated = stage_dil > 1;
            const int stride = (b == 0 && l > 0 && !dilated) ? 2 : 1;
            const int oh = ch / stride, ow = cw / stride, pl = planes[l], outc = pl * expansion;
            auto conv_bn = [&](const std::string& name, const std::string& bn, int src, int cin, int cout, int k, int st, int hi, int wi, bool frozen, int cg) {
                Unit u = B.conv_unit(name, "", bn, src, cin, cout, k, st, hi, wi, cg);
                u.frozen_candidate = frozen; u.cg = cg;
                if (dilated && k == 3) { u.dil = stage_dil; u.pad = stage_dil; }
                return u;
            };
            // the block's convolutions in torchvision's registration order (= state_dict order): conv1 bn1 conv2 bn2 [conv3 bn3]
            // [downsample.0 downsample.1].  BasicBlock: 3x3 (stride) - 3x3; Bottleneck (v1.5): 1x1 - 3x3 (stride) - 1x1 (x4).
            // All of them are described - and their outputs allocated - before the first is emitted; the downsample comes after.
            std::vector<Unit> us;
            if (!bottleneck) {
                us.push_back(conv_bn(pre + ".conv1.weight", pre + ".bn1", cur, inpl, pl, 3, stride, ch, cw, true, 0));
                us.push_back(conv_bn(pre + ".conv2.weight", pre + ".bn2", us[0].out, pl, pl, 3, 1, oh, ow, true, 0));
            } else {
                const int width = groups > 1 ? pl * 2 : pl;
                us.push_back(conv_bn(pre + ".conv1.weight", pre + ".bn1", cur, inpl, width, 1, 1, ch, cw, true, 0));
                us.push_back(conv_bn(pre + ".conv2.weight", pre + ".bn2", us[0].out, width, width, 3, stride, ch, cw, true,
                                     groups > 1 ? width / groups : 0));
                us.push_back(conv_bn(pre + ".conv3.weight", pre + ".bn3", us[1].out, width, outc, 1, 1, oh, ow, true, 0));
            }
            Unit& last = us.back();
            for (size_t q = 0; q + 1 < us.size(); ++q) B.emit(us[q]);
            if (stride != 1 || inpl != outc || (dilated && b == 0)) {   // "downsample" lacks "conv" in its name: not frozen by the reference's predicate
                Unit ud = conv_bn(pre + ".downsample.0.weight", pre + ".downsample.1", cur, inpl, outc, 1, stride, ch, cw, false, 0);
                ud.relu = 0;
                last.res = B.emit(ud);
            } else {
                last.res = cur;
            }
            cur = B.emit(last); inpl = outc; ch = oh; cw = ow;
        }
        f.feat[l + 2] = cur;
        f.featc[l + 2] = inpl;
    }
    return f;
}

// ---- decoders ----
// smp's DecoderBlock on cat(nearest-x2(x), skips): Conv3x3 + BN + ReLU twice.  Its tensors, in state-dict order ..
struct DecoderBlockTensors { int w1, bn1, w2, bn2; };
DecoderBlockTensors decoder_block_tensors(Builder& B, const std::string& pre, int cin, int cout) {
    DecoderBlockTensors t;
    t.w1 = B.weight(pre + ".conv1.0.weight", {cout, cin, 3, 3}); t.bn1 = B.bn(pre + ".conv1.1", cout);
    t.w2 = B.weight(pre + ".conv2.0.weight", {cout, cout, 3, 3}); t.bn2 = B.bn(pre + ".conv2.1", cout);
    return t;
}
// .. and its units.  conv1 reads up(x) ++ skip through its loader (up0; `skips` = at most ONE activation of skip_c channels, already
// concatenated where there were several) when the boundary x_c is a multiple of 32 channels; where it is not (EfficientNet features of
// 136 / 56 / 48 channels) cat([nearest-x2(x), skips...]) is materialised as ONE activation (U_UP2 + U_CONCAT) and conv1 reads that.
// conv1_act_first: conv1's output is allocated before the materialised concatenation's two activations (MA-Net describes conv1
// first), not after them (U-Net++).  Returns conv2's output.
int decoder_block(Builder& B, const DecoderBlockTensors& t, int x_act, int x_c, const std::vector<int>& skips, int skip_c, int cout,
                  bool conv1_act_first = false) {
    const int oh = 2 * B.A[x_act].h, ow = 2 * B.A[x_act].w;
    Unit u1 = Builder::conv(x_act, x_c + skip_c, cout, 3, 1, oh, ow);
    u1.w_idx = t.w1; u1.bn_idx = t.bn1;
    if (conv1_act_first) u1.out = B.act(cout, oh, ow, true);
    if (!skips.empty() && x_c % 32 != 0) {
        const int up = B.op(U_UP2, x_act, -1, x_c, oh / 2, ow / 2, oh, ow).out;
        std::vector<int> members = {up};
        members.insert(members.end(), skips.begin(), skips.end());
        u1.src0 = B.concat(members, x_c + skip_c, oh, ow);
    } else {
        u1.up0 = 1; u1.cin0 = x_c; u1.cin1 = skip_c; u1.src1 = skips.empty() ? -1 : skips[0];
    }
    if (!conv1_act_first) u1.out = B.act(cout, oh, ow, true);
    Unit u2 = Builder::conv(u1.out, cout, cout, 3, 1, oh, ow);
    u2.w_idx = t.w2; u2.bn_idx = t.bn2;
    u2.out = B.act(cout, oh, ow, true);
    B.emit(u1);
    return B.emit(u2);
}
const int kDecoderChannels[5] = {256, 128, 64, 32, 16};   // smp's default decoder_channels

HeadInput decoder_unet(Builder& B, const Features& f) {
    const int* dec = kDecoderChannels;
    int x = f.feat[5], xc = f.featc[5];
    for (int i = 0; i < 5; ++i) {
        const int skip_c = i < 4 ? f.featc[4 - i] : 0;
        const DecoderBlockTensors t = decoder_block_tensors(B, "decoder.blocks." + std::to_string(i), xc + skip_c, dec[i]);
        x = decoder_block(B, t, x, xc, skip_c ? std::vector<int>{f.feat[4 - i]} : std::vector<int>{}, skip_c, dec[i]);
        xc = dec[i];
    }
    return {x, xc, 3, 1};
}

HeadInput decoder_unetplusplus(Builder& B, const Features& f) {
    // smp.UnetPlusPlusDecoder (decoders/unetplusplus/decoder.py of segmentation-models-pytorch 0.2.1, restated):
    // features reversed, deepest first: f[0] = layer4 .. f[4] = stem; in_channels = [C(f0), 256, 128, 64, 32],
    // skip_channels = [C(f1), C(f2), C(f3), C(f4), 0], out_channels = dec.  Node x_d_l = DecoderBlock(up(x_d_(l-1) or f[d]),
    // cat(x_(d+1)_l .. x_l_l, f[l+1])); all nodes x_*_l and f[l+1] share a resolution.  Parameters are REGISTERED in the
    // constructor's order (x_0_0; x_0_1 x_1_1; x_0_2 x_1_2 x_2_2; ..; x_0_4) but EXECUTED in forward()'s order
    // (x_0_0 x_1_1 x_2_2 x_3_3; x_0_1 x_1_2 x_2_3; x_0_2 x_1_3; x_0_3; x_0_4): tensors first, units second.
    const int* dec = kDecoderChannels;
    const int f_act[5] = {f.feat[5], f.feat[4], f.feat[3], f.feat[2], f.feat[1]};
    const int f_c[5] = {f.featc[5], f.featc[4], f.featc[3], f.featc[2], f.featc[1]};
    const int skipc[5] = {f_c[1], f_c[2], f_c[3], f_c[4], 0};
    const int in_c[5] = {f_c[0], dec[0], dec[1], dec[2], dec[3]};
    struct Node { int skip_ch, out_ch, out_act; DecoderBlockTensors t; };
    Node node[5][5] = {};
    auto reg = [&](int d, int l, int in_ch, int skip_ch, int out_ch) {
        node[d][l].skip_ch = skip_ch; node[d][l].out_ch = out_ch;
        node[d][l].t = decoder_block_tensors(B, "decoder.blocks.x_" + std::to_string(d) + "_" + std::to_string(l), in_ch + skip_ch, out_ch);
    };
    for (int l = 0; l < 4; ++l)
        for (int d = 0; d <= l; ++d) {
            if (d == 0) reg(0, l, in_c[l], skipc[l] * (l + 1), dec[l]);
            else reg(d, l, skipc[l - 1], skipc[l] * (l + 1 - d), skipc[l]);
        }
    reg(0, 4, in_c[4], 0, dec[4]);
    auto run_node = [&](int d, int l, int x_act, int x_c, std::vector<int> skips) {
        Node& nd = node[d][l];
        // on the loader's route the concatenation of the skips is materialised (channel-slice copies, also for a single member): its gradient is split back
        if (!skips.empty() && x_c % 32 == 0) skips = {B.concat(skips, nd.skip_ch, 2 * B.A[x_act].h, 2 * B.A[x_act].w)};
        nd.out_act = decoder_block(B, nd.t, x_act, x_c, skips, nd.skip_ch, nd.out_ch);
    };
    for (int layer = 0; layer < 4; ++layer)
        for (int d = 0; d < 4 - layer; ++d) {
            const int l = d + layer;
            if (layer == 0) {
                run_node(d, d, f_act[d], f_c[d], {f_act[d + 1]});
            } else {
                std::vector<int> members;
                for (int idx = d + 1; idx <= l; ++idx) members.push_back(node[idx][l].out_act);
                members.push_back(f_act[l + 1]);
                run_node(d, l, node[d][l - 1].out_act, node[d][l - 1].out_ch, members);
            }
        }
    run_node(0, 4, node[0][3].out_act, node[0][3].out_ch, {});
    return {node[0][4].out_act, dec[4], 3, 1};
}

HeadInput decoder_linknet(Builder& B, const Features& f) {
    // smp.Linknet (decoders/linknet/decoder.py of segmentation-models-pytorch 0.2.1, restated): channels = reversed encoder
    // features (deepest first) + [32]; block i = Conv2dReLU(in, in/4, 1) -> TransposeX2(in/4, in/4) -> Conv2dReLU(in/4, out, 1),
    // then + skip (the next-shallower encoder feature) for i < 4; head = Conv2d(32, classes, 1).
    const int chans[6] = {f.featc[5], f.featc[4], f.featc[3], f.featc[2], f.featc[1], 32};
    const int skips[5] = {f.feat[4], f.feat[3], f.feat[2], f.feat[1], -1};
    int x = f.feat[5], xh = B.A[x].h, xw = B.A[x].w;
    for (int i = 0; i < 5; ++i) {
        const std::string pre = "decoder.blocks." + std::to_string(i) + ".block.";
        const int cin = chans[i], mid = cin / 4, cout = chans[i + 1];
        x = B.emit(B.conv_unit(pre + "0.0.weight", "", pre + "0.1", x, cin, mid, 1, 1, xh, xw));
        Unit ut = Builder::conv(x, mid, mid, 3, 1, xh, xw);
        ut.kind = U_CONVT; ut.hout = 2 * xh; ut.wout = 2 * xw;
        ut.w_idx = B.tensor(pre + "1.0.weight", {mid, mid, 4, 4}, 3);   // torch's [in][out][kh][kw], as is
        B.attach_bias(ut, pre + "1.0.bias");
        B.attach_bn(ut, pre + "1.1");
        ut.out = B.act(mid, 2 * xh, 2 * xw, true);
        x = B.emit(ut);
        xh *= 2; xw *= 2;
        x = B.emit(B.conv_unit(pre + "2.0.weight", "", pre + "2.1", x, mid, cout, 1, 1, xh, xw));
        if (skips[i] >= 0) x = B.op(U_ADD, x, skips[i], cout, 0, 0, xh, xw).out;
    }
    return {x, 32, 1, 1};
}

HeadInput decoder_fpn(Builder& B, const Features& f) {
    // smp.FPN (decoders/fpn/decoder.py of segmentation-models-pytorch 0.2.1, restated): p5 = Conv1x1(c5); p_k = nearest-x2(p_(k+1)) +
    // Conv1x1(c_k) for k = 4, 3, 2 (pyramid_channels 256, biased, no norm); seg_blocks[i] on p5, p4, p3, p2 with 3, 2, 1, 0
    // upsamplings: Conv3x3(256 -> 128, no bias) + GroupNorm(32) + ReLU (+ bilinear x2, align_corners) then (ups - 1) x
    // [Conv3x3(128 -> 128) + GN + ReLU + bilinear x2]; merge = sum; Dropout2d(0.2); head = Conv1x1(128 -> classes) +
    // UpsamplingBilinear2d(4).
    const int pyr = 256, seg = 128;
    auto lateral = [&](const std::string& name, int src, int cin) {
        Unit u = B.conv_unit(name + ".weight", name + ".bias", "", src, cin, pyr, 1, 1, B.A[src].h, B.A[src].w);
        u.relu = 0;
        return B.emit(u);
    };
    int pyramid[4];
    pyramid[0] = lateral("decoder.p5", f.feat[5], f.featc[5]);
    for (int k = 0; k < 3; ++k) {   // p4, p3, p2
        const int lat = lateral("decoder.p" + std::to_string(4 - k) + ".skip_conv", f.feat[4 - k], f.featc[4 - k]);
        const Act la = B.A[lat];
        pyramid[k + 1] = B.op(U_UPADD, pyramid[k], lat, pyr, la.h / 2, la.w / 2, la.h, la.w).out;
    }
    int merged = -1;
    for (int i = 0; i < 4; ++i) {
        const int ups = 3 - i;
        int x = pyramid[i], x_c = pyr;
        for (int j = 0; j < std::max(1, ups); ++j) {
            const std::string pre = "decoder.seg_blocks." + std::to_string(i) + ".block." + std::to_string(j) + ".block.";
            const Act xa = B.A[x];
            Unit u = Builder::conv(x, x_c, seg, 3, 1, xa.h, xa.w);
            B.attach_weight(u, pre + "0.weight");
            B.attach_gn(u, pre + "1", 32);
            u.out = B.act(seg, xa.h, xa.w, true);
            x = B.emit(u); x_c = seg;
            if (ups > 0) x = B.op(U_BILINEAR, x, -1, seg, xa.h, xa.w, 2 * xa.h, 2 * xa.w).out;
        }
        merged = merged < 0 ? x : B.op(U_ADD, merged, x, seg, 0, 0, B.A[merged].h, B.A[merged].w).out;
    }
    const int dropped = B.op(U_DROPOUT, merged, -1, seg, 0, 0, B.A[merged].h, B.A[merged].w).out;
    return {dropped, seg, 1, 4};
}

// smp's ASPP(C5, 256, rates (12, 24, 36)) + Dropout(0.5) on the deepest feature, tensors under `pre`: convs = [1x1 conv + BN + ReLU,
// 3 x branch(prefix of convs.r, rate), ASPPPooling = Sequential(AdaptiveAvgPool2d(1), Conv2d, BatchNorm2d, ReLU) + F.interpolate(size,
// bilinear, align_corners=False) back to the map], concat, project = 1x1 conv (1280 -> 256) + BN + ReLU + Dropout(0.5).
// conv_bn(wname, bnname, src, cin, cout, h, w, k) and branch(prefix, rate) are the caller's: dense dilated 3x3 (DeepLabV3) / separable (DeepLabV3+)
template <class ConvBn, class Branch>
int aspp(Builder& B, const std::string& pre, const Features& f, ConvBn conv_bn, Branch branch) {
    const int c5 = f.feat[5], c5c = f.featc[5], ah = B.A[c5].h, aw = B.A[c5].w;
    std::vector<int> branches;
    branches.push_back(conv_bn(pre + ".convs.0.0.weight", pre + ".convs.0.1", c5, c5c, 256, ah, aw, 1));
    const int rates[3] = {12, 24, 36};
    for (int r = 0; r < 3; ++r) branches.push_back(branch(pre + ".convs." + std::to_string(r + 1), rates[r]));
    const int pooled = conv_bn(pre + ".convs.4.1.weight", pre + ".convs.4.2", B.gap(c5, c5c, ah, aw), c5c, 256, 1, 1, 1);
    branches.push_back(B.op(U_BCAST, pooled, -1, 256, 1, 1, ah, aw).out);
    const int cat = B.concat(branches, 5 * 256, ah, aw);
    const int proj = conv_bn(pre + ".project.0.weight", pre + ".project.1", cat, 5 * 256, 256, ah, aw, 1);
    return B.op(U_DROPOUT_E, proj, -1, 256, 0, 0, ah, aw).out;
}

HeadInput decoder_deeplabv3(Builder& B, const Features& f) {
    // smp.DeepLabV3 (decoders/deeplabv3/decoder.py, restated; encoder_output_stride 8): DeepLabV3Decoder = Sequential(ASPP(C5, 256,
    // rates (12, 24, 36)), Conv2d(256, 256, 3, padding=1, bias=False), BatchNorm2d, ReLU); ASPP as in DeepLabV3+ but with DENSE
    // dilated 3x3 branches (ASPPConv); head = Conv2d(256, classes, 1) + UpsamplingBilinear2d(8).
    const int c5 = f.feat[5], c5c = f.featc[5], ah = B.A[c5].h, aw = B.A[c5].w;
    auto conv_bn = [&](const std::string& wname, const std::string& bnname, int src, int cin, int cout, int hh, int ww, int k, int rate = 0) {
        Unit u = B.conv_unit(wname, "", bnname, src, cin, cout, k, 1, hh, ww);
        u.colr = rate;
        return B.emit(u);
    };
    const int dropped = aspp(B, "decoder.0", f, conv_bn,
                             [&](const std::string& pre, int rate) { return conv_bn(pre + ".0.weight", pre + ".1", c5, c5c, 256, ah, aw, 3, rate); });
    return {conv_bn("decoder.1.weight", "decoder.2", dropped, 256, 256, ah, aw, 3), 256, 1, 8};
}

HeadInput decoder_deeplabv3plus(Builder& B, const Features& f) {
    // smp.DeepLabV3Plus (decoders/deeplabv3/decoder.py of segmentation-models-pytorch 0.2.1, restated; encoder_output_stride 16:
    // layer4 dilated above).  aspp = Sequential(ASPP(C5, 256, rates (12, 24, 36), separable), SeparableConv2d(256, 256, 3), BN,
    // ReLU); ASPP: convs = [1x1 conv + BN + ReLU, 3 x (SeparableConv2d(C5, 256, 3, dilation r) + BN + ReLU), AdaptiveAvgPool2d(1)
    // + 1x1 conv + BN + ReLU + bilinear back to the map], concat, project = 1x1 conv (1280 -> 256) + BN + ReLU + Dropout(0.5);
    // up = UpsamplingBilinear2d(4); block1 = 1x1 conv (C2 -> 48) + BN + ReLU on the stride-4 feature; concat; block2 =
    // SeparableConv2d(304, 256, 3) + BN + ReLU; head = Conv2d(256, classes, 1) + UpsamplingBilinear2d(4).
    // SeparableConv2d = depthwise 3x3 (dilation = padding) then pointwise 1x1, no norm in between, both without bias.
    const int c5 = f.feat[5], c5c = f.featc[5], ah = B.A[c5].h, aw = B.A[c5].w;
    auto conv_bn = [&](const std::string& wname, const std::string& bnname, int src, int cin, int cout, int hh, int ww, int k) {
        return B.emit(B.conv_unit(wname, "", bnname, src, cin, cout, k, 1, hh, ww));
    };
    auto separable_bn = [&](const std::string& pre_conv, const std::string& bnname, int src, int cin, int cout, int hh, int ww, int dil) {
        Unit d; d.kind = U_DWCONV; d.src0 = src; d.cin0 = cin; d.cout = cin; d.k = 3; d.dil = dil; d.pad = dil; d.relu = 0;
        d.hin = hh; d.win = ww; d.hout = hh; d.wout = ww;
        d.w_idx = B.weight(pre_conv + ".0.weight", {cin, 1, 3, 3});
        d.out = B.act(cin, hh, ww, false);
        // the pointwise convolution's weight follows the depthwise one in the state dict, its BatchNorm after both
        const Unit u = B.conv_unit(pre_conv + ".1.weight", "", bnname, d.out, cin, cout, 1, 1, hh, ww);
        B.emit(d);
        return B.emit(u);
    };
    const int dropped = aspp(B, "decoder.aspp.0", f, conv_bn,
                             [&](const std::string& pre, int rate) { return separable_bn(pre + ".0", pre + ".1", c5, c5c, 256, ah, aw, rate); });
    const int deep = separable_bn("decoder.aspp.1", "decoder.aspp.2", dropped, 256, 256, ah, aw, 1);
    Unit& up = B.op(U_BILINEAR, deep, -1, 256, ah, aw, 4 * ah, 4 * aw);
    up.factor = 4;
    const int up_act = up.out;
    const Act hr = B.A[f.feat[2]];
    const int high = conv_bn("decoder.block1.0.weight", "decoder.block1.1", f.feat[2], f.featc[2], 48, hr.h, hr.w, 1);
    const int cat2 = B.concat({up_act, high}, 256 + 48, hr.h, hr.w);
    return {separable_bn("decoder.block2.0", "decoder.block2.1", cat2, 256 + 48, 256, hr.h, hr.w, 1), 256, 1, 4};
}

HeadInput decoder_manet(Builder& B, const Features& f) {
    // smp.MAnet (decoders/manet/decoder.py of segmentation-models-pytorch 0.2.1, restated): center = PAB(C5, pab_channels 64):
    // top / center 1x1 convs (C5 -> 64), bottom 3x3 conv (C5 -> C5), all biased, attention (vs_pab_attention_*), out_conv 3x3
    // (biased).  blocks[i] = MFAB(in, skip, out, reduction 16) for the four levels with a skip: hl_conv = Conv3x3(in, in) + BN +
    // ReLU, Conv1x1(in, skip) + BN + ReLU; nearest x2; SE_hl on it, SE_ll on the skip (AdaptiveAvgPool2d(1), Conv1x1(skip,
    // skip / 16), ReLU, Conv1x1(-> skip), Sigmoid); x * (SE_hl + SE_ll); cat skip; conv1, conv2 (3x3 + BN + ReLU);
    // blocks[4] = U-Net's DecoderBlock(32, 0, 16).  The gate commutes with the nearest upsampling, so it is applied at the
    // low resolution and conv1 reads up(x * gate) ++ skip through its loader, as the U-Net decoder does.
    const int C5 = f.featc[5];
    const Act fa = B.A[f.feat[5]];
    auto plain = [&](const std::string& name, int src, int cin, int cout, int k) {
        Unit u = B.conv_unit(name + ".weight", name + ".bias", "", src, cin, cout, k, 1, fa.h, fa.w);
        u.relu = 0;
        return B.emit(u);
    };
    const int top = plain("decoder.center.top_conv", f.feat[5], C5, 64, 1);
    const int cen = plain("decoder.center.center_conv", f.feat[5], C5, 64, 1);
    const int bot = plain("decoder.center.bottom_conv", f.feat[5], C5, C5, 3);
    Unit& pab = B.op(U_PAB, f.feat[5], -1, C5, 0, 0, fa.h, fa.w);
    pab.members = {top, cen, bot}; pab.cin0 = 64;
    int x = plain("decoder.center.out_conv", pab.out, C5, C5, 3), x_c = C5, xh = fa.h, xw = fa.w;
    const int* dec = kDecoderChannels;
    for (int i = 0; i < 5; ++i) {
        const std::string pre = "decoder.blocks." + std::to_string(i);
        const int S = i < 4 ? f.featc[4 - i] : 0, skip = i < 4 ? f.feat[4 - i] : -1;
        if (S > 0) {
            const int h0 = B.emit(B.conv_unit(pre + ".hl_conv.0.0.weight", "", pre + ".hl_conv.0.1", x, x_c, x_c, 3, 1, xh, xw));
            const int h1 = B.emit(B.conv_unit(pre + ".hl_conv.1.0.weight", "", pre + ".hl_conv.1.1", h0, x_c, S, 1, 1, xh, xw));
            const int R = std::max(1, S / 16);
            const int w_ll = B.se_tensors(pre + ".SE_ll.1", pre + ".SE_ll.3", S, R);      // registration order: ll, then hl
            const int w_hl = B.se_tensors(pre + ".SE_hl.1", pre + ".SE_hl.3", S, R);
            const int a_hl = B.se(B.gap(h1, S, xh, xw), S, R, w_hl, 0);
            const int a_ll = B.se(B.gap(skip, S, 2 * xh, 2 * xw), S, R, w_ll, 0);
            const int gate = B.op(U_ADD, a_hl, a_ll, S, 0, 0, 1, 1).out;
            x = B.op(U_CGATE, h1, gate, S, 0, 0, xh, xw).out; x_c = S;
        }
        const DecoderBlockTensors t = decoder_block_tensors(B, pre, x_c + S, dec[i]);
        x = decoder_block(B, t, x, x_c, S > 0 ? std::vector<int>{skip} : std::vector<int>{}, S, dec[i], true);
        x_c = dec[i]; xh *= 2; xw *= 2;
    }
    return {x, 16, 3, 1};
}

HeadInput decoder_pan(Builder& B, const Features& f) {
    // smp.PAN (decoders/pan/decoder.py of segmentation-models-pytorch 0.2.1, restated; decoder_channels 32, encoder_dilation).
    // ConvBnRelu = biased Conv2d + BatchNorm2d (+ ReLU).  FPABlock(C5, 32): branch1 = AdaptiveAvgPool2d(1) + ConvBnRelu 1x1
    // (broadcast back), mid = ConvBnRelu 1x1, the single-channel pyramid (down1 .. conv1, vs_fpa_pyramid_*), out = plane * mid +
    // branch1.  GAUBlock(Ck, 32)(x, y): conv1 = AdaptiveAvgPool2d(1) + ConvBnRelu 1x1 without ReLU + Sigmoid on y, conv2 =
    // ConvBnRelu 3x3 on x; out = bilinear(y -> x's size) + conv2(x) * conv1(y).  gau3 / gau2 / gau1 on the stride-16 / 8 / 4
    // features; head = Conv2d(32, classes, 3, padding 1) + UpsamplingBilinear2d(4).
    const int C5 = f.featc[5];
    const Act fa = B.A[f.feat[5]];
    // described, not emitted: the convolutions' tensors are registered and their outputs allocated in the constructor's order, ahead of
    // the pools that feed them and run first
    auto cbr_bias = [&](const std::string& pre, int src, int cin, int cout, int k, int hh, int ww, int relu) {
        Unit u = B.conv_unit(pre + ".conv.weight", pre + ".conv.bias", pre + ".bn", src, cin, cout, k, 1, hh, ww);
        u.relu = relu;
        return u;
    };
    // ---- FPA ----
    Unit b1 = cbr_bias("decoder.fpa.branch1.1", -1, C5, 32, 1, 1, 1, 1);
    Unit mid = cbr_bias("decoder.fpa.mid.0", f.feat[5], C5, 32, 1, fa.h, fa.w, 1);
    Unit fpa; fpa.kind = U_FPA; fpa.src0 = f.feat[5]; fpa.cin0 = C5; fpa.cout = 32; fpa.hin = fa.h; fpa.win = fa.w; fpa.hout = fa.h; fpa.wout = fa.w; fpa.relu = 0;
    {
        const char* names[6] = {"decoder.fpa.down1.1", "decoder.fpa.down2.1", "decoder.fpa.down3.1", "decoder.fpa.down3.2", "decoder.fpa.conv2", "decoder.fpa.conv1"};
        const int ks[6] = {7, 5, 3, 3, 5, 7};
        for (int i = 0; i < 6; ++i) {
            fpa.tens.push_back(B.weight(std::string(names[i]) + ".conv.weight", {1, i == 0 ? C5 : 1, ks[i], ks[i]}));
            fpa.tens.push_back(B.bias(std::string(names[i]) + ".conv.bias", 1));
            const int g = B.bn(std::string(names[i]) + ".bn", 1);
            fpa.tens.push_back(g); fpa.tens.push_back(g + 1);
        }
        fpa.w_idx = fpa.tens[0];
    }
    b1.src0 = B.gap(f.feat[5], C5, fa.h, fa.w);
    fpa.res = B.emit(b1);
    fpa.src1 = B.emit(mid);
    fpa.out = B.act(32, fa.h, fa.w, false);
    // ---- GAU x 3 ----
    int y = B.emit(fpa);
    for (int i = 0; i < 3; ++i) {
        const std::string pre = "decoder.gau" + std::to_string(3 - i);
        const int gx = f.feat[4 - i];
        const Act xa = B.A[gx], ya = B.A[y];
        Unit c1 = cbr_bias(pre + ".conv1.1", -1, 32, 32, 1, 1, 1, 0);      // registered first, as in smp's constructor
        Unit c2 = cbr_bias(pre + ".conv2", gx, f.featc[4 - i], 32, 3, xa.h, xa.w, 1);
        c1.src0 = B.gap(y, 32, ya.h, ya.w);
        const int gate = B.op(U_SIGMOID, B.emit(c1), -1, 32, 0, 0, 1, 1).out;
        const int gated = B.op(U_CGATE, B.emit(c2), gate, 32, 0, 0, xa.h, xa.w).out;
        Unit& up = B.op(U_BILINEAR, y, -1, 32, ya.h, ya.w, xa.h, xa.w);
        up.factor = xa.h / ya.h;
        y = B.op(U_ADD, up.out, gated, 32, 0, 0, xa.h, xa.w).out;
    }
    return {y, 32, 3, 4};
}

int build_plan(vs_unet* net) {
    Builder B(net);
    const Features f = (net->encoder == 103 || net->encoder == 104) ? encoder_efficientnet(B)
                       : (net->encoder == 150 || net->encoder == 201) ? encoder_resnest(B) : encoder_resnet(B);
    HeadInput x{};
    switch (net->topology) {
        case 0: x = decoder_unet(B, f); break;
        case 1: x = decoder_unetplusplus(B, f); break;
        case 2: x = decoder_linknet(B, f); break;
        case 3: x = decoder_fpn(B, f); break;
        case 4: x = decoder_deeplabv3plus(B, f); break;
        case 5: x = decoder_deeplabv3(B, f); break;
        case 6: x = decoder_manet(B, f); break;
        default: x = decoder_pan(B, f); break;
    }
    net->head_up = x.up;     // the head works at 1 / head_up resolution, nn.UpsamplingBilinear2d(head_up) follows
    Unit head = Builder::conv(x.act, x.c, net->classes, x.k, 1, B.A[x.act].h, B.A[x.act].w);
    head.kind = U_HEAD; head.relu = 0;
    B.attach_weight(head, "segmentation_head.0.weight");
    B.attach_bias(head, "segmentation_head.0.bias");
    B.emit(head);
    return VS_OK;
}

size_t plan_workspace(vs_unet* net) {
    const size_t N = (size_t)net->max_batch, esz = net->esz;
    size_t off = 0;
    // (skewing the tensors' offsets against one another - 4 KB, 68 KB, 1 MB steps - was measured: no effect on the step; what looked like a placement effect was
    // the side stream's hardware queue, see acquire_side_streams in unet.hip)
    auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return o; };
    // weight copies + BN constants
    size_t ct = 0;
    for (auto& u : net->units) {
        if (u.kind == U_CONV || u.kind == U_HEAD || u.kind == U_CONVT) {
            const WeightCopyBytes b = weight_copy_bytes(u, esz);
            u.off_wc = take(b.wc);
            u.off_wt = take(b.wt);
        }
        if (u.kind == U_CONVT) ct = std::max(ct, N * u.hin * u.win * 4 * u.cout * esz);
        if (u.bn_idx >= 0) u.off_bn = take(4 * (size_t)u.cout * sizeof(float));
    }
    net->off_ct = take(ct);    // the transposed convolutions' un-shuffled output
    for (auto& u : net->units) {
        if (u.kind != U_FPA) continue;
        u.off_fpa_pool = take(2 * N * (u.hin / 2) * (u.win / 2) * u.cin0 * esz);     // the pooled input and (backward) its gradient
        u.off_fpa_arena = take(vs_fpa_arena_floats((int)N, u.hin, u.win) * sizeof(float));
        u.off_fpa_plane = take(2 * N * u.hin * u.win * sizeof(float));     // the plane and (backward) its gradient
    }
    {
        size_t pab = 0, sews = 0, gapws = 0;
        for (auto& u : net->units) {
            if (u.kind == U_PAB) {
                const size_t hw = (size_t)u.hout * u.wout;
                u.off_gn = take(N * hw * hw * sizeof(float));                       // the attention map, kept for the backward pass
                pab = std::max(pab, vs_pab_scratch_bytes((int)N, (int)hw, u.cout));
            }
            if (u.kind == U_SE) u.off_gn = take(N * (size_t)u.cin1 * sizeof(float));   // hidden activations
            if (u.kind == U_SE) sews = std::max(sews, vs_se_gate_scratch_floats((int)N, u.cout, u.cin1) * sizeof(float));
            if (u.kind == U_GAP || u.kind == U_CGATE) gapws = std::max(gapws, vs_sample_rowsum_workspace((int)N, u.cout));
            if (u.kind == U_RADIXSUM) gapws = std::max(gapws, vs_sample_rowsum_workspace((int)N, 2 * u.cout));
            if (u.kind == U_DROPADD) u.off_gn = take(N * sizeof(float));               // the drop-connect draw per sample
        }
        net->pab_bytes = pab;
        net->off_pab = take(pab);
        net->off_sews = take(sews);
        for (auto& u : net->units)
            if (u.kind == U_AVGPOOL) net->avgw_c = std::max(net->avgw_c, u.cout);
        net->off_avgw9 = take((size_t)net->avgw_c * 9 * sizeof(float));
        net->off_avgw4 = take((size_t)net->avgw_c * 4 * sizeof(float));
        net->gapws_bytes = gapws;
        net->off_gapws = take(gapws);
    }
    {
        size_t ys = 0;
        for (auto& u : net->units) {
            if (u.kind != U_CONV || !u.colr) continue;
            const size_t col = N * u.hin * u.win * 9 * u.cin0 * esz;
            u.off_xs = take(col);
            ys = std::max(ys, col);
        }
        net->off_ys = take(ys);
    }
    {   // smp.FPN: GroupNorm statistics per unit, a scratch for the pre-norm convolution output in evaluation (training keeps z),
        // the reduction workspace, the quarter-resolution logits in front of the head's bilinear upsampling
        size_t gnz = 0, gnws = 0;
        for (auto& u : net->units) {
            if (u.kind != U_CONV || u.gn_idx < 0) continue;
            u.off_gn = take((size_t)2 * N * u.gn_groups * sizeof(float));
            gnz = std::max(gnz, N * u.hout * u.wout * u.cout * esz);
            gnws = std::max(gnws, vs_gn_bwd_workspace((int)N, u.cout, u.gn_groups));
        }
        net->off_gnz = take(gnz);
        net->gnws_bytes = gnws;
        net->off_gnws = take(gnws);
        const Unit& hd = net->units.back();
        net->off_lsmall = take(net->head_up > 1 ? N * net->classes * (size_t)hd.hout * hd.wout * sizeof(float) : 0);
    }
    int cmax = 512;
    for (auto& u : net->units) cmax = std::max(cmax, u.cout);
    net->bnws_bytes = 4 * vs_bn_workspace(0, cmax);  // also receives the conv epilogue's per-tile statistics
    net->off_bnws = take(net->bnws_bytes);
    net->off_bncnt = take(256);                      // reserved, unused (zeroed by vs_unet_prepare): taking them out moves every later offset
    net->off_syncsc = take((size_t)2 * cmax * sizeof(float));
    {   // fixed-point statistics bins of every convolution + BatchNorm unit (ConvParams::stats_bins): one contiguous block
        size_t total = 0;
        for (auto& u : net->units)
            if (has_stat_bins(u)) total += unit_bins_bytes(u.cout) + kTicketBytes;
        net->bins_bytes = total;
        net->off_bins0 = take(total);
        size_t at = net->off_bins0;
        for (auto& u : net->units)
            if (has_stat_bins(u)) { u.off_bins = at; at += unit_bins_bytes(u.cout) + kTicketBytes; }
    }
    // activations (a for all, z for conv/stem outputs)
    for (auto& a : net->acts) {
        const size_t bytes = N * a.c * a.h * a.w * esz;
        a.off_a = take(bytes);
    }
    net->off_logits = take(N * net->classes * (size_t)net->h * net->w * sizeof(float));   // vs_unet_forward_to_volume's fallback path
    net->ws_eval = off;
    size_t ctdw = 0;
    for (auto& u : net->units) {
        if (u.kind == U_CONVT) ctdw = std::max(ctdw, (size_t)4 * u.cout * 9 * u.cin0 * sizeof(float));
        if (u.kind == U_CONV && u.g2) ctdw = std::max(ctdw, (size_t)u.cout * u.k * u.k * u.cin0 * sizeof(float));
        if (u.kind != U_CONV && u.kind != U_HEAD && u.kind != U_CONVT) continue;
        const WeightCopyBytes b = weight_copy_bytes(u, esz);
        u.off_wc2 = take(b.wc);
        u.off_wt2 = take(b.wt);
    }
    {
        const Unit& hd = net->units.back();
        net->off_dlsmall = take(net->head_up > 1 ? N * net->classes * (size_t)hd.hout * hd.wout * sizeof(float) : 0);
        size_t dm = 0;
        for (auto& u : net->units)
            if (u.kind == U_DROPOUT) dm = std::max(dm, N * u.cout * sizeof(float));
        net->off_dropmask = take(dm);
    }
    net->ctdw_bytes = ctdw;
    net->off_ctdw = take(ctdw * vs_unet::kSide);   // dense weight gradient of a transposed convolution's 3x3 form, per side stream
    for (auto& a : net->acts) {
        const size_t bytes = N * a.c * a.h * a.w * esz;
        if (a.has_z) { a.off_z = take(bytes); a.off_dz = take(bytes); }
        a.off_da = take(bytes);
    }
    // wgrad split-K slabs: worst case over layers
    size_t wg = vs_stem_wgrad_workspace((int)N, net->h, net->w);
    for (auto& u : net->units) {
        if (u.kind != U_CONV && u.kind != U_HEAD && u.kind != U_CONVT) continue;
        WgradParams p{};
        p.C0 = u.cin0; p.C1 = u.cin1; p.up0 = u.up0; p.N = (int)N; p.Hin = u.hin; p.Win = u.win;
        p.Hout = u.hout; p.Wout = u.wout; p.stride = u.stride; p.pad = u.pad; p.KH = p.KW = u.k;
        p.Cout = u.kind == U_HEAD ? 16 : u.cout;
        if (u.kind == U_CONVT) { p.Hout = u.hin; p.Wout = u.win; p.Cout = 4 * u.cout; }
        p.cg = u.cg; p.dil = u.dil;
        if (u.colr) { p.C0 = 9 * u.cin0; p.pad = 0; p.KH = p.KW = 1; }
        const size_t b = wgrad_workspace_bytes(net->dtype, p);
        if (b > wg) wg = b;
    }
    for (auto& u : net->units) {
        if (u.kind == U_DWCONV) wg = std::max(wg, vs_dwconv3x3_wgrad_workspace(u.cout));
        if (u.kind == U_DWCONV2) wg = std::max(wg, vs_dwconv2d_wgrad_workspace(u.cout, u.k));
    }
    net->wgws_bytes = wg;
    net->off_wgws = take(wg * vs_unet::kSide);  // one slab workspace per side stream
    {
        const Unit& hd = net->units.back();
        net->off_headdw = take((size_t)16 * hd.k * hd.k * hd.cin0 * sizeof(float));
        net->off_headpart = take((size_t)1024 * 16 * sizeof(float));   // bias-gradient partials of the head's conversion sweep when it runs on the side stream
    }
    net->off_dyh = take(N * net->h * net->w * 16 * esz);
    size_t dup = 0, zs = 0;
    for (auto& u : net->units) {
        if (u.kind != U_CONV) continue;
        if (u.up0) dup = std::max(dup, N * u.hin * u.win * u.cin0 * esz);
        if (u.stride == 2) zs = std::max(zs, N * u.hin * u.win * u.cout * esz);
    }
    net->off_dup = take(dup);
    net->off_zs = take(zs);
    {
        size_t idx = 0;      // the max-pool's argmax bytes (one per output element; 64 channels for the ResNets, 128 for timm-resnest101e's stem)
        for (auto& u : net->units)
            if (u.kind == U_POOL) idx = std::max(idx, N * (size_t)u.hout * u.wout * u.cout);
        net->off_idx = take(idx);
    }
    net->ws_train = off;
    return off;
}

// ---- parameter table -------------------------------------------------------------------------------
// the (topology, encoder) pairs that are built; encoder_code = topology * 1000 + encoder, `who` heads the message
int check_network_code(const char* who, int encoder_code) {
    const int encoder = encoder_code % 1000, topology = encoder_code / 1000;
    VS_REQUIRE(topology >= 0 && topology <= 7, "%s: topology must be 0 (U-Net), 1 (U-Net++), 2 (Linknet), 3 (FPN), 4 (DeepLabV3+), 5 (DeepLabV3), 6 (MA-Net) or 7 (PAN), got %d", who, topology);
    VS_REQUIRE(encoder == 18 || encoder == 34 || encoder == 50 || encoder == 51 || encoder == 103 || encoder == 104 || encoder == 150 || encoder == 201,
               "%s: encoder must be 18, 34, 50, 51, 103, 104, 150 or 201 (resnet18 / resnet34 / resnet50 / resnext50_32x4d / efficientnet-b3 / "
               "efficientnet-b4 / timm-resnest50d / timm-resnest101e), got %d", who, encoder);
    VS_REQUIRE((encoder != 103 && encoder != 104) || topology != 2,
               "%s: the EfficientNet encoders are not built under smp.Linknet (its decoder narrows 56 / 48 channels to 14 / 12: not multiples of 8)", who);
    VS_REQUIRE((encoder != 150 && encoder != 201) || (topology != 4 && topology != 5 && topology != 7),
               "%s: the ResNeSt encoders do not support the dilating decoders (DeepLabV3 / DeepLabV3+ / PAN) - smp's ResNestEncoder.make_dilated "
               "raises for them as well (their parameter-free average pools would stay at stride 2)", who);
    return VS_OK;
}

int with_layout(int classes, int encoder_code, Layout& out) {
    vs_unet tmp{};
    if (check_network_code("unet_tensor_info", encoder_code)) return VS_ERR_INVALID;
    VS_REQUIRE(classes >= 1 && classes <= 16, "classes must be in [1,16], got %d", classes);
    tmp.classes = classes; tmp.h = 64; tmp.w = 64; tmp.max_batch = 1; tmp.dtype = VS_F32; tmp.esz = 4;
    tmp.encoder = encoder_code % 1000; tmp.topology = encoder_code / 1000;
    build_plan(&tmp);
    out = tmp.layout;
    return VS_OK;
}

}  // namespace

// ---- the activation graph (the one function the passes call here) -----------------------------------
// producer / consumer maps of the activation graph (built once)
void unet::ensure_graph_maps(vs_unet* net) {
    if (!net->producer.empty()) return;
    net->producer.assign(net->acts.size(), -1);
    net->first_consumer.assign(net->acts.size(), 1 << 30);
    net->sole_consumer.assign(net->acts.size(), -1);
    std::vector<int> readers(net->acts.size(), 0);
    for (int k = 0; k < (int)net->units.size(); ++k) {
        const Unit& v = net->units[k];
        if (v.out >= 0) net->producer[v.out] = k;
        auto reads = [&](int a) {
            if (a < 0) return;
            if (k < net->first_consumer[a]) net->first_consumer[a] = k;
            ++readers[a];
            net->sole_consumer[a] = k;
        };
        for (int a : {v.src0, v.src1, v.res}) reads(a);
        for (int a : v.members) reads(a);
    }
    for (size_t a = 0; a < readers.size(); ++a)
        if (readers[a] != 1) net->sole_consumer[a] = -1;
}

// ---- parameter table: the C entry points --------------------------------------------------------------
extern "C" int vs_unet_num_tensors_ex(int classes, int encoder) {
    Layout L;
    if (with_layout(classes, encoder, L)) return VS_ERR_INVALID;
    return (int)L.tensors.size();
}
extern "C" int vs_unet_num_tensors(int classes) { return vs_unet_num_tensors_ex(classes, 34); }

extern "C" int vs_unet_tensor_info_ex(int classes, int encoder, int index, char* name, int name_len, int64_t shape[4], int* ndim,
                                      int* kind, int64_t* offset) {
    Layout L;
    if (with_layout(classes, encoder, L)) return VS_ERR_INVALID;
    VS_REQUIRE(index >= 0 && index < (int)L.tensors.size(), "tensor index %d out of range", index);
    const TensorInfo& t = L.tensors[index];
    if (name && name_len > 0) { strncpy(name, t.name.c_str(), name_len - 1); name[name_len - 1] = 0; }
    for (int i = 0; i < 4; ++i) shape[i] = t.shape[i];
    *ndim = t.ndim; *kind = t.kind; *offset = t.offset;
    return VS_OK;
}

extern "C" int vs_unet_tensor_info(int classes, int index, char* name, int name_len, int64_t shape[4], int* ndim,
                                   int* kind, int64_t* offset) {
    return vs_unet_tensor_info_ex(classes, 34, index, name, name_len, shape, ndim, kind, offset);
}

extern "C" int64_t vs_unet_param_elems_ex(int classes, int encoder) {
    Layout L;
    if (with_layout(classes, encoder, L)) return -1;
    return L.n_params;
}
extern "C" int64_t vs_unet_param_elems(int classes) { return vs_unet_param_elems_ex(classes, 34); }

extern "C" int64_t vs_unet_bnstate_elems_ex(int classes, int encoder) {
    Layout L;
    if (with_layout(classes, encoder, L)) return -1;
    return L.n_bnstate;
}
extern "C" int64_t vs_unet_bnstate_elems(int classes) { return vs_unet_bnstate_elems_ex(classes, 34); }

// ---- lifecycle -------------------------------------------------------------------------------------
extern "C" int vs_unet_create(vs_unet_t** out, int dtype, int classes, int max_batch, int h, int w) {
    return vs_unet_create_ex(out, dtype, classes, max_batch, h, w, 34);
}

extern "C" int vs_unet_create_ex(vs_unet_t** out, int dtype, int classes, int max_batch, int h, int w, int encoder_code) {
    VS_REQUIRE(out, "unet_create: null out pointer");
    if (check_network_code("unet_create", encoder_code)) return VS_ERR_INVALID;
    VS_REQUIRE(dtype == VS_F32 || dtype == VS_BF16 || dtype == VS_F16, "unet_create: bad dtype %d", dtype);
    VS_REQUIRE(classes >= 1 && classes <= 16, "unet_create: classes must be in [1,16], got %d", classes);
    VS_REQUIRE(max_batch >= 1 && h >= 32 && w >= 32 && h % 32 == 0 && w % 32 == 0,
               "unet_create: batch %d, %dx%d - spatial dims must be positive multiples of 32", max_batch, h, w);
    vs_unet* net = new vs_unet();
    net->dtype = dtype; net->classes = classes; net->max_batch = max_batch; net->h = h; net->w = w;
    net->encoder = encoder_code % 1000;
    net->topology = encoder_code / 1000;
    net->esz = dtype_size(dtype);
    build_plan(net);
    plan_workspace(net);
    *out = net;
    return VS_OK;
}

extern "C" void vs_unet_destroy(vs_unet_t* net) { delete net; }

extern "C" size_t vs_unet_workspace_bytes(const vs_unet_t* net, int training) {
    return training ? net->ws_train : net->ws_eval;
}

// ---- where a pass leaves what: mask and parameter offsets ---------------------------------------------
// byte offset inside the training workspace of the last training forward's Dropout2d mask ([n][128] fp32), -1 without dropout (tests)
extern "C" int64_t vs_unet_dropout_mask_offset(const vs_unet_t* net) {
    if (!net) return -1;
    for (auto& u : net->units)
        if (u.kind == U_DROPOUT) return (int64_t)net->off_dropmask;
    return -1;
}
// the drop-connect draws of the last training forward (EfficientNet encoders): for every MBConv block with a skip and a non-zero rate,
// its block index, rate and the byte offset in the training workspace of its [n] fp32 mask (0 or 1 / keep); returns their number (tests)
extern "C" int vs_unet_drop_connect_masks(const vs_unet_t* net, int64_t* offsets, int* blocks, float* rates, int cap) {
    if (!net) return 0;
    int k = 0;
    for (auto& u : net->units) {
        if (u.kind != U_DROPADD || u.drop_p <= 0.f) continue;
        if (k < cap) { if (offsets) offsets[k] = (int64_t)u.off_gn; if (blocks) blocks[k] = u.salt; if (rates) rates[k] = u.drop_p; }
        ++k;
    }
    return k;
}

// first tensor-table index (parameter-buffer element offset) owned by a unit: lets a caller map unit ranges to slices
extern "C" int64_t vs_unet_unit_param_offset(const vs_unet_t* net, int unit) {
    if (!net || unit < 0 || unit > (int)net->units.size()) return -1;
    if (unit == (int)net->units.size()) return net->layout.n_params;
    for (int u = unit; u < (int)net->units.size(); ++u)
        if (net->units[u].w_idx >= 0) return net->layout.tensors[net->units[u].w_idx].offset;
    return net->layout.n_params;
}

// ---- debug: locate a unit's tensors inside the workspace (tests / diagnostics only) ----------------------
extern "C" int vs_unet_num_units(const vs_unet_t* net) { return (int)net->units.size(); }
extern "C" int vs_unet_debug_unit(const vs_unet_t* net, int unit, char* wname, int name_len, int* c, int* h, int* w,
                                  size_t* off_a, size_t* off_z, size_t* off_da, size_t* off_dz) {
    VS_REQUIRE(net && unit >= 0 && unit < (int)net->units.size(), "debug_unit: bad index");
    const Unit& u = net->units[unit];
    const char* nm = u.w_idx >= 0 ? net->layout.tensors[u.w_idx].name.c_str() : u.kind == U_BN ? net->layout.tensors[u.bn_idx].name.c_str() : u.kind == U_DROPADD ? "drop_connect+add" : u.kind == U_RADIXSUM ? "radix-weighted sum" : u.kind == U_FOLD2 ? "radix fold" : u.kind == U_RSOFTMAX ? "radix softmax" : u.kind == U_AVGPOOL ? "avgpool k" : (u.kind == U_CONCAT ? "concat" : (u.kind == U_ADD ? "add" : (u.kind == U_UPADD ? "upsample+add" : (u.kind == U_BILINEAR ? "bilinear"
                         : (u.kind == U_DROPOUT ? "dropout2d" : (u.kind == U_GAP ? "avgpool" : (u.kind == U_BCAST ? "broadcast" : (u.kind == U_DROPOUT_E ? "dropout"
                         : (u.kind == U_PAB ? "pab attention" : (u.kind == U_CGATE ? "channel gate" : (u.kind == U_SIGMOID ? "sigmoid" : "maxpool")))))))))));
    strncpy(wname, nm, name_len - 1); wname[name_len - 1] = 0;
    if (u.out < 0) { *c = *h = *w = 0; *off_a = *off_z = *off_da = *off_dz = 0; return VS_OK; }
    const Act& a = net->acts[u.out];
    *c = a.c; *h = a.h; *w = a.w; *off_a = a.off_a; *off_z = a.off_z; *off_da = a.off_da; *off_dz = a.off_dz;
    return VS_OK;
}

// ---- plan dump -------------------------------------------------------------------------------------
// The whole plan as line-oriented text, every value as name=value: one header line, one line per tensor, per activation and per
// unit, with EVERY member of Unit (also those a kind never reads; floats as %a).  Host only; it reads and nothing else.  Two builds
// construct the same plans exactly when their dumps are equal byte for byte (tools/unet_plan_sweep.py, tests/test_host_logic.py).
extern "C" size_t vs_unet_plan_dump(const vs_unet_t* net, char* buf, size_t cap) {
    if (!net) return 0;
    std::string s;
    char tmp[160];
    auto I = [&](const char* name, long long v) { snprintf(tmp, sizeof tmp, " %s=%lld", name, v); s += tmp; };
    auto Z = [&](const char* name, size_t v) { snprintf(tmp, sizeof tmp, " %s=%zu", name, v); s += tmp; };
    auto F = [&](const char* name, float v) { snprintf(tmp, sizeof tmp, " %s=%a", name, (double)v); s += tmp; };
    auto list = [&](const char* name, const std::vector<int>& v) {
        s += " "; s += name; s += "=[";
        for (size_t i = 0; i < v.size(); ++i) { if (i) s += ","; s += std::to_string(v[i]); }
        s += "]";
    };
    s += "plan";
    I("dtype", net->dtype); I("classes", net->classes); I("max_batch", net->max_batch); I("h", net->h); I("w", net->w);
    I("topology", net->topology); I("encoder", net->encoder); I("head_up", net->head_up); Z("esz", net->esz);
    I("n_params", net->layout.n_params); I("n_bnstate", net->layout.n_bnstate); Z("ws_eval", net->ws_eval); Z("ws_train", net->ws_train);
    Z("off_bins0", net->off_bins0); Z("bins_bytes", net->bins_bytes); Z("off_bnws", net->off_bnws); Z("bnws_bytes", net->bnws_bytes);
    Z("off_wgws", net->off_wgws); Z("wgws_bytes", net->wgws_bytes); Z("off_headdw", net->off_headdw); Z("off_headpart", net->off_headpart);
    Z("off_dyh", net->off_dyh); Z("off_dup", net->off_dup); Z("off_zs", net->off_zs); Z("off_idx", net->off_idx);
    Z("off_logits", net->off_logits); Z("off_bncnt", net->off_bncnt); Z("off_syncsc", net->off_syncsc); Z("off_gnz", net->off_gnz);
    Z("off_gnws", net->off_gnws); Z("gnws_bytes", net->gnws_bytes); Z("off_dropmask", net->off_dropmask); Z("off_lsmall", net->off_lsmall);
    Z("off_dlsmall", net->off_dlsmall); Z("off_pab", net->off_pab); Z("pab_bytes", net->pab_bytes); Z("off_sews", net->off_sews);
    Z("off_gapws", net->off_gapws); Z("gapws_bytes", net->gapws_bytes); Z("off_avgw9", net->off_avgw9); Z("off_avgw4", net->off_avgw4);
    I("avgw_c", net->avgw_c); Z("off_ys", net->off_ys); Z("off_ct", net->off_ct); Z("off_ctdw", net->off_ctdw); Z("ctdw_bytes", net->ctdw_bytes);
    s += "\n";
    for (size_t i = 0; i < net->layout.tensors.size(); ++i) {
        const TensorInfo& t = net->layout.tensors[i];
        s += "tensor";
        I("index", (long long)i); s += " name=" + t.name; I("ndim", t.ndim);
        s += " shape=[";
        for (int d = 0; d < 4; ++d) { if (d) s += ","; s += std::to_string(t.shape[d]); }
        s += "]";
        I("kind", t.kind); I("offset", t.offset);
        s += "\n";
    }
    for (size_t i = 0; i < net->acts.size(); ++i) {
        const Act& a = net->acts[i];
        s += "act";
        I("index", (long long)i); I("c", a.c); I("h", a.h); I("w", a.w); I("has_z", a.has_z);
        Z("off_a", a.off_a); Z("off_z", a.off_z); Z("off_da", a.off_da); Z("off_dz", a.off_dz);
        s += "\n";
    }
    for (size_t i = 0; i < net->units.size(); ++i) {
        const Unit& u = net->units[i];
        s += "unit";
        I("index", (long long)i); I("kind", u.kind); I("src0", u.src0); I("src1", u.src1); I("up0", u.up0);
        I("cin0", u.cin0); I("cin1", u.cin1); I("cout", u.cout); I("k", u.k); I("stride", u.stride); I("pad", u.pad);
        I("hin", u.hin); I("win", u.win); I("hout", u.hout); I("wout", u.wout);
        I("w_idx", u.w_idx); I("bn_idx", u.bn_idx); I("bias_idx", u.bias_idx); I("out", u.out); I("res", u.res); I("relu", u.relu);
        I("gn_idx", u.gn_idx); I("gn_groups", u.gn_groups); Z("off_gn", u.off_gn); F("bn_eps", u.bn_eps); F("bn_mom", u.bn_mom);
        F("drop_p", u.drop_p); I("salt", u.salt); I("bcast", u.bcast); I("g2", u.g2); I("aux_frozen", u.aux_frozen); F("pool_w", u.pool_w);
        I("dil", u.dil); I("factor", u.factor); I("colr", u.colr); Z("off_xs", u.off_xs); I("cg", u.cg);
        I("frozen_candidate", u.frozen_candidate); Z("off_wc", u.off_wc); Z("off_wt", u.off_wt); Z("off_bn", u.off_bn);
        Z("off_bins", u.off_bins); Z("off_wc2", u.off_wc2); Z("off_wt2", u.off_wt2); list("tens", u.tens);
        Z("off_fpa_pool", u.off_fpa_pool); Z("off_fpa_arena", u.off_fpa_arena); Z("off_fpa_plane", u.off_fpa_plane);
        list("members", u.members);
        s += "\n";
    }
    if (buf && cap) memcpy(buf, s.data(), std::min(cap, s.size()));
    return s.size();
}
