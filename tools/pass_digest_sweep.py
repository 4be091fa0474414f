#!/usr/bin/env python3
"""What the network passes compute, digested - the device-side companion of unet_plan_sweep.py.  Needs a GPU.

    python tools/pass_digest_sweep.py LIB [--out FILE] [--option NAME=VALUE]...
    python tools/pass_digest_sweep.py LIB --kinds          (host only: which unit kinds the listed networks reach)

LIB is a libvolseg_hip.so; --option sets a runtime option of it (vs_set_option) before anything runs.  For each network of NETWORKS, with seeded parameters, input and dropout draws (vs_unet_set_rng): one
evaluation forward (bf16) and, in fp32 and in bf16, two fused training steps (vs_unet_forward in training mode +
vs_unet_backward_adamw; the first with the encoder frozen, the second without).  Batch 2 at 64 x 64 (128 x 128 under the dilating
decoders).  One line per network and precision with the SHA-256 of the evaluation logits, of both steps' training logits, of both
steps' flat gradient buffers, of the parameters and of the BatchNorm state after the second step.  The kernels are deterministic: two
builds enqueue the same launches with the same arguments exactly when every line matches.  One invocation opens one library;
comparing two builds is two invocations and a diff.  The networks together reach every unit kind (checked before anything runs).
"""
import ctypes as C
import hashlib
import re
import sys

import torch  # before the library: its dependency on the HIP runtime must resolve to torch's copy

ENCODERS = {"resnet34": 34, "resnet50": 50, "resnext50_32x4d": 51, "efficientnet-b3": 103, "timm-resnest50d": 150}
TOPOLOGIES = {"unet": 0, "unetplusplus": 1, "linknet": 2, "fpn": 3, "deeplabv3plus": 4, "deeplabv3": 5, "manet": 6, "pan": 7}
NETWORKS = (("unet", "resnet34"), ("unetplusplus", "resnet34"), ("linknet", "resnet34"), ("fpn", "resnet34"), ("deeplabv3plus", "resnet34"),
            ("deeplabv3", "resnet50"), ("manet", "resnet34"), ("pan", "resnet34"), ("unet", "efficientnet-b3"), ("unet", "timm-resnest50d"),
            ("unet", "resnext50_32x4d"), ("unetplusplus", "efficientnet-b3"))     # (the last: the one with a materialised upsampling, U_UP2)
N_KINDS = 27          # csrc/unet_plan.h: enum UnitKind
CLASSES, BATCH = 3, 2
P, I = C.c_void_p, C.c_int


def load(path):
    lib = C.CDLL(str(path))
    for name, res, args in (
            ("vs_last_error", C.c_char_p, []), ("vs_unet_create_ex", I, [C.POINTER(P)] + [I] * 6), ("vs_unet_destroy", None, [P]),
            ("vs_unet_plan_dump", C.c_size_t, [P, C.c_char_p, C.c_size_t]), ("vs_unet_num_tensors_ex", I, [I, I]),
            ("vs_unet_tensor_info_ex", I, [I, I, I, C.c_char_p, I, C.POINTER(C.c_int64), C.POINTER(I), C.POINTER(I), C.POINTER(C.c_int64)]),
            ("vs_unet_param_elems_ex", C.c_int64, [I, I]), ("vs_unet_bnstate_elems_ex", C.c_int64, [I, I]),
            ("vs_unet_workspace_bytes", C.c_size_t, [P, I]), ("vs_unet_prepare", I, [P, P, P, I, P, P]),
            ("vs_unet_forward", I, [P, P, P, P, I, I, P, P, P]), ("vs_unet_backward_adamw", I, [P, P, P, I, I, P, P, P, P]),
            ("vs_unet_set_rng", I, [P, C.c_uint32, P]), ("vs_set_option", I, [C.c_char_p, I])):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


class AdamwArgs(C.Structure):
    _fields_ = [("params", P), ("exp_avg", P), ("exp_avg_sq", P), ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float),
                ("eps", C.c_float), ("weight_decay", C.c_float), ("step", C.c_int32), ("hyper", P)]


def check(lib, rc):
    if rc:
        raise RuntimeError(lib.vs_last_error().decode())


def size_of(topology):
    return 128 if topology in ("deeplabv3plus", "deeplabv3", "pan") else 64


def create(lib, dtype, code, size):
    net = P()
    check(lib, lib.vs_unet_create_ex(C.byref(net), dtype, CLASSES, BATCH, size, size, code))
    return net


def kinds_reached(lib):
    """the unit kinds in the plans of NETWORKS (host only)"""
    kinds = set()
    buf = C.create_string_buffer(1 << 21)
    for topology, encoder in NETWORKS:
        net = create(lib, 1, TOPOLOGIES[topology] * 1000 + ENCODERS[encoder], size_of(topology))
        need = lib.vs_unet_plan_dump(net, buf, len(buf))
        assert need <= len(buf), need
        kinds |= {int(k) for k in re.findall(rb"^unit index=\d+ kind=(\d+)", buf.raw[:need], re.M)}
        lib.vs_unet_destroy(net)
    return kinds


def seeded_state(lib, code):
    """(params, bnstate) on the host: every tensor of the state dict from one seeded generator, scaled by its role"""
    g = torch.Generator().manual_seed(1000 + code)
    params = torch.empty(lib.vs_unet_param_elems_ex(CLASSES, code))
    bnstate = torch.empty(lib.vs_unet_bnstate_elems_ex(CLASSES, code))
    name = C.create_string_buffer(160)
    shape, ndim, kind, off = (C.c_int64 * 4)(), I(), I(), C.c_int64()
    for i in range(lib.vs_unet_num_tensors_ex(CLASSES, code)):
        check(lib, lib.vs_unet_tensor_info_ex(CLASSES, code, i, name, len(name), shape, C.byref(ndim), C.byref(kind), C.byref(off)))
        dims = [shape[d] for d in range(ndim.value)]
        numel = 1
        for d in dims:
            numel *= d
        r = torch.randn(numel, generator=g)
        if kind.value in (0, 3) and len(dims) == 4:      # a convolution weight: He scale
            v = r * (2.0 / (numel / dims[0])) ** 0.5
        elif kind.value == 1:                             # norm weight
            v = 1.0 + 0.1 * r
        elif kind.value == 5:                             # running variance
            v = 1.0 + 0.2 * r.abs()
        else:                                             # norm bias, bias, running mean
            v = 0.1 * r
        (params if kind.value <= 3 else bnstate)[off.value:off.value + numel] = v
    return params, bnstate


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()[:32]


def run(lib, topology, encoder, dtype):
    """the digest line of one network in one precision (dtype 0 fp32 / 1 bf16)"""
    dev = "cuda:0"
    code, size = TOPOLOGIES[topology] * 1000 + ENCODERS[encoder], size_of(topology)
    params_h, bnstate_h = seeded_state(lib, code)
    params, bnstate = params_h.to(dev), bnstate_h.to(dev)
    g = torch.Generator().manual_seed(7)
    x = torch.randn(BATCH, 1, size, size, generator=g).to(dev)
    dlogits = (1e-3 * torch.randn(BATCH, CLASSES, size, size, generator=g)).to(dev)
    logits = torch.zeros(BATCH, CLASSES, size, size, device=dev)
    grads, m, v = torch.zeros_like(params), torch.zeros_like(params), torch.zeros_like(params)
    counter = torch.zeros(1, dtype=torch.int64, device=dev)
    net = create(lib, dtype, code, size)
    ws = torch.zeros(lib.vs_unet_workspace_bytes(net, 1), dtype=torch.uint8, device=dev)
    ptr = lambda t: t.data_ptr()
    check(lib, lib.vs_unet_set_rng(net, 1234, ptr(counter)))
    fields = []
    if dtype == 1:
        check(lib, lib.vs_unet_prepare(net, ptr(params), ptr(bnstate), 0, ptr(ws), None))
        check(lib, lib.vs_unet_forward(net, ptr(params), ptr(bnstate), ptr(x), BATCH, 0, ptr(logits), ptr(ws), None))
        torch.cuda.synchronize()
        fields.append(("eval", sha(logits)))
    check(lib, lib.vs_unet_prepare(net, ptr(params), ptr(bnstate), 1, ptr(ws), None))
    train_logits, step_grads = [], []
    for step in (1, 2):
        counter.fill_(step)
        check(lib, lib.vs_unet_forward(net, ptr(params), ptr(bnstate), ptr(x), BATCH, 1, ptr(logits), ptr(ws), None))
        opt = AdamwArgs(ptr(params), ptr(m), ptr(v), 1e-3, 0.9, 0.999, 1e-8, 1e-2, step, None)
        check(lib, lib.vs_unet_backward_adamw(net, ptr(x), ptr(dlogits), BATCH, step - 1, ptr(grads), ptr(ws), None, C.byref(opt)))
        torch.cuda.synchronize()
        train_logits.append(logits.clone())
        step_grads.append(grads.clone())
    fields += [("train", sha(*train_logits)), ("grads", sha(*step_grads)), ("params", sha(params)), ("bnstate", sha(bnstate))]
    finite = all(bool(torch.isfinite(t).all()) for t in train_logits + step_grads + [params, bnstate])
    lib.vs_unet_destroy(net)
    return f"{topology}/{encoder} {'bf16' if dtype else 'fp32'} " + " ".join(f"{k}={d}" for k, d in fields) + ("" if finite else " NOT-FINITE")


def main():
    args = sys.argv[1:]
    out = None
    if "--out" in args:
        i = args.index("--out")
        out = args[i + 1]
        del args[i:i + 2]
    kinds_only = "--kinds" in args
    if kinds_only:
        args.remove("--kinds")
    options = []
    while "--option" in args:
        i = args.index("--option")
        name, _, value = args[i + 1].partition("=") if i + 1 < len(args) else ("", "", "")
        if not name or not value.lstrip("-").isdigit():
            sys.exit(__doc__)
        options.append((name, int(value)))
        del args[i:i + 2]
    if len(args) != 1:
        sys.exit(__doc__)
    lib = load(args[0])
    for name, value in options:
        if lib.vs_set_option(name.encode(), value):
            sys.exit(f"vs_set_option({name}) failed: {lib.vs_last_error().decode()}")
    kinds = kinds_reached(lib)
    missing = sorted(set(range(N_KINDS)) - kinds)
    assert not missing, f"the listed networks never reach the unit kinds {missing}"
    if kinds_only:
        print(f"{len(NETWORKS)} networks reach all {N_KINDS} unit kinds")
        return
    assert torch.cuda.is_available(), "the pass digests need a GPU"
    lines = []
    for topology, encoder in NETWORKS:
        for dtype in (0, 1):
            lines.append(run(lib, topology, encoder, dtype))
            print(lines[-1], flush=True)
    total = hashlib.sha256("\n".join(lines).encode()).hexdigest()
    lines.append(f"== {len(NETWORKS)} networks x fp32 / bf16, sha256 {total}")
    print(lines[-1])
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
