"""Phase stamps of the training step's convolution launches in their TRAINING forms (needs a GPU) - the companion of
tools/conv_probe.py, which times the plain forward form only.

    [VOLSEG_HIP_LIB=<other build>/libvolseg_hip.so] python tools/conv_rounds_probe.py

Per layer shape of the batch-32 step and per epilogue form - plain store, plain + residual (in place), the fused BatchNorm-backward
epilogue with the mask from y and earlier contributions (the form of most data gradients) and with the mask recomputed - one launch
with vs_debug_probe set after a few warm ones: the median over the workgroups of entry -> first chunk in LDS, the main loop, and end
of loop -> stores acknowledged (100 MHz stamps), and the launch time from HIP events over back-to-back launches."""
import ctypes as C
import pathlib
import sys

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))
sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1] / "tests"))
import numpy as np
import torch

import hip_helpers as H

L = H.lib()
DEV = "cuda:0"
N = 32


def run(name, hw, c, form, reps=200):
    d = H.conv_desc(L, 1, N, hw, hw, c, c, 3, 1, 1)
    t = L.ConvTrain()
    bf = dict(device=DEV, dtype=torch.bfloat16)
    x = torch.randn(N, hw, hw, c, device=DEV).bfloat16()
    w = (torch.randn(c, 9, c, device=DEV) * 0.05).bfloat16()
    z, y = torch.randn(N, hw, hw, c, **bf), torch.randn(N, hw, hw, c, **bf)
    out = torch.randn(N, hw, hw, c, **bf)
    vec = [torch.randn(c, device=DEV), torch.rand(c, device=DEV) + 0.5, torch.rand(c, device=DEV) + 0.5, torch.randn(c, device=DEV)]
    res = None
    if form in ("bnbwd-y", "bnbwd-z"):
        t.bz, t.bmean, t.binvstd, t.brelu = z.data_ptr(), vec[0].data_ptr(), vec[1].data_ptr(), 1
        if form == "bnbwd-y":
            t.by = y.data_ptr()
        else:
            t.bgamma, t.bbeta = vec[2].data_ptr(), vec[3].data_ptr()
        part = torch.zeros(L.lib.vs_conv2d_stat_rows(d, t), 2, c, device=DEV)
        t.bstats_partial = part.data_ptr()
    if form in ("bnbwd-y", "residual"):
        res = out.data_ptr()
    code = L.lib.vs_conv2d_train_variant(d, t)
    st = L.stream_ptr()
    call = lambda: L.check(L.lib.vs_conv2d_train(d, x.data_ptr(), None, w.data_ptr(), res, out.data_ptr(), None, C.byref(t), st))
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        call()
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / reps
    if code % 10 == 7:      # the persistent stream kernel stamps per job, not per workgroup (tools/stream_probe.py reads those)
        print(f"{name:8s} {hw:3d}x{hw:<3d} {c:3d}ch plan {code} {form:9s}: {us:6.1f} us/launch", flush=True)
        return
    cap = 1 << 16
    buf = torch.zeros(cap * 8, dtype=torch.int64, device=DEV)
    med = []
    for _ in range(5):
        buf.zero_()
        L.check(L.lib.vs_debug_probe(L.ptr(buf), cap))
        call()
        torch.cuda.synchronize()
        L.check(L.lib.vs_debug_probe(None, 0))
        b = buf.cpu().numpy().reshape(cap, 8)
        b = b[b[:, 0] != 0]
        tt = b[:, :5].astype(np.float64) * 0.01
        med.append([np.median(tt[:, 1] - tt[:, 0]), np.median(tt[:, 3] - tt[:, 1]), np.median(tt[:, 4] - tt[:, 3]), np.median(tt[:, 4] - tt[:, 0]), len(b)])
    m = np.median(np.array(med), axis=0)
    print(f"{name:8s} {hw:3d}x{hw:<3d} {c:3d}ch plan {code} {form:9s}: {us:6.1f} us/launch | workgroup medians (5 probed launches): head {m[0]:5.2f}  loop {m[1]:5.2f}  "
          f"tail {m[2]:5.2f}  life {m[3]:5.2f} us  ({int(m[4])} WGs)", flush=True)


if __name__ == "__main__":
    for name, hw, c in (("layer1", 64, 64), ("layer2", 32, 128), ("layer3", 16, 256), ("layer4", 8, 512)):
        for form in ("plain", "residual", "bnbwd-y", "bnbwd-z"):
            run(name, hw, c, form)
