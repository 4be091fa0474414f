"""Time of the confusion-matrix kernel (vs_confusion_matrix, csrc/evaluate.hip) on 512^3 label volumes next to the route a user had
before it - torch.bincount(t.long() * K + p.long(), minlength=K * K) on the device - and to the read-only streaming rate of this
box measured in the same run by the method of tools/hbm_probe.py (needs a GPU).  HIP events around each call, warm-up first, median
of the repeats; the kernel's result is compared with the torch route's at the timed size.

    python tools/evaluate_probe.py [--out profiles/evaluate_confusion.txt] [--repeats 20]

Conditions checked at the end (exit status 1 when one fails): in every case the kernel is faster than the torch route, which moves at
least eight times the bytes; and the coherent volume is not slower than uniform random labels - if it is, the aggregation in front of
the LDS atomics is not working."""
import argparse
import pathlib
import statistics
import sys

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))
import numpy as np
import torch

from volume_segmantics_amd import _lib as L
from volume_segmantics_amd.utilities import base_data_utils as U

REPO = pathlib.Path(__file__).resolve().parents[1]
DEV = "cuda:0"
SIDE = 512


def median_ms(fn, warmup=3, repeats=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times), min(times), max(times)


def streaming_rate():
    """bytes/s of a read-only pass over 1 GiB (tools/hbm_probe.py: torch's own sum of a bf16 tensor)"""
    x = torch.randn(1 << 29, device=DEV, dtype=torch.bfloat16)
    ms, _, _ = median_ms(lambda: x.sum(), repeats=10)
    return x.numel() * 2 / (ms * 1e-3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "evaluate_confusion.txt"))
    ap.add_argument("--repeats", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("evaluate_probe: no GPU - nothing here is measured on a host")

    n = SIDE ** 3
    g = torch.Generator(device=DEV).manual_seed(0)
    labels = np.tile(U.numpy_from_hdf5(REPO / "tests" / "golden" / "vessels_256cube_LABELS.h5", "/data")[0], (2, 2, 2))
    values = np.unique(labels)
    vessels = torch.from_numpy(np.searchsorted(values, labels).astype(np.uint8)).to(DEV).reshape(-1)
    shifted = torch.roll(vessels.reshape(SIDE, SIDE, SIDE), shifts=(1, 1, 1), dims=(0, 1, 2)).contiguous().reshape(-1)
    kv = max(len(values), 2)
    rand = {k: (torch.randint(0, k, (n,), device=DEV, dtype=torch.uint8, generator=g),
                torch.randint(0, k, (n,), device=DEV, dtype=torch.uint8, generator=g)) for k in (4, 16)}
    cases = [("1 uniform random, K = 4, whole volume", *rand[4], 4, n),
             (f"2 vessels 2x2x2 vs shifted by one voxel, K = {kv}, whole volume", vessels, shifted, kv, n),
             ("3 uniform random, K = 16, whole volume", *rand[16], 16, n),
             (f"4 vessels 2x2x2 vs shifted, K = {kv}, per slice (512 slabs)", vessels, shifted, kv, SIDE * SIDE)]

    stream = streaming_rate()
    lines = [f"vs_confusion_matrix on {SIDE}^3 uint8 label volumes ({torch.cuda.get_device_name(0)}); HIP events, 3 warm-up calls, "
             f"median of {args.repeats} (min .. max); a call = two memsets + the kernel",
             f"read-only streaming rate of this box in this run (torch sum over 1 GiB, tools/hbm_probe.py): {stream / 1e12:.2f} TB/s",
             "bytes read = 2 per voxel; 256 MiB in all, which the 256 MiB Infinity Cache can hold in part between repeats: the rates are "
             "those of repeated calls on resident volumes, not of a cold first pass"]
    results = {}
    for name, t, p, k, slab in cases:
        nslabs = n // slab
        counts = torch.empty((nslabs, k, k), dtype=torch.int64, device=DEV)
        dropped = torch.empty((nslabs, 2), dtype=torch.int64, device=DEV)

        def kernel():
            L.check(L.lib.vs_confusion_matrix(L.ptr(t), L.ptr(p), n, k, None, slab, L.ptr(counts), L.ptr(dropped), L.stream_ptr()))

        offset = None if nslabs == 1 else (torch.arange(nslabs, device=DEV) * (k * k)).repeat_interleave(slab)

        def torch_route():
            code = t.long() * k + p.long()
            return torch.bincount(code if offset is None else code + offset, minlength=nslabs * k * k)

        k_ms, k_lo, k_hi = median_ms(kernel, repeats=args.repeats)
        t_ms, t_lo, t_hi = median_ms(torch_route, repeats=max(3, args.repeats // 4))
        same = bool(torch.equal(counts.reshape(-1), torch_route())) and int(dropped.sum()) == 0
        rate = 2 * n / (k_ms * 1e-3)
        results[name[0]] = (k_ms, t_ms, same)
        lines.append(f"case {name}: kernel {k_ms:.3f} ms ({k_lo:.3f} .. {k_hi:.3f}), {rate / 1e12:.2f} TB/s read = {rate / stream:.2f} of the "
                     f"streaming rate | torch.bincount route {t_ms:.2f} ms ({t_lo:.2f} .. {t_hi:.2f}) = {t_ms / k_ms:.0f}x | "
                     f"counts {'equal' if same else 'DIFFER'}")
        print(lines[-1], flush=True)

    ok_faster = all(k_ms < t_ms for k_ms, t_ms, _ in results.values())
    ok_coherent = results["2"][0] <= results["1"][0]
    ok_same = all(s for _, _, s in results.values())
    lines.append(f"conditions: kernel faster than the torch route in every case: {'yes' if ok_faster else 'NO'}; coherent (case 2) not slower than "
                 f"random (case 1): {'yes' if ok_coherent else 'NO'} ({results['2'][0]:.3f} vs {results['1'][0]:.3f} ms); results equal: "
                 f"{'yes' if ok_same else 'NO'}")
    text = "\n".join(lines) + "\n"
    print(text)
    out = pathlib.Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(text)
    sys.exit(0 if ok_faster and ok_coherent and ok_same else 1)


if __name__ == "__main__":
    main()
