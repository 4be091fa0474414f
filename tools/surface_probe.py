"""Times of the surface-distance kernels (csrc/surface.hip: vs_label_surface, the three passes of vs_edt_squared,
vs_surface_distance_histogram) on 512^3 label volumes, next to the read-only streaming rate of this box measured in the same run by
the method of tools/hbm_probe.py and - where scipy imports - to scipy.ndimage.distance_transform_edt on the host for the same volume
(needs a GPU).  HIP events around each call, warm-up first, median of the repeats; the passes of the transform are timed by the
library's own profile records (x, y, z in launch order).  One class, one direction per case: the evaluation runs this once per class
and direction.

    python tools/surface_probe.py [--out profiles/surface_distances.txt] [--repeats 10] [--no-scipy]

Cases: the vessels labels tiled 2x2x2 against themselves shifted by one voxel (surfaces near each other: short searches); uniform
random labels, K = 4 (nearly every voxel a surface voxel); a single-voxel class (the outward search runs the whole axis for every
voxel: its worst case).  Exit status 1 when a histogram total differs from the surface count or the device transform differs from
scipy's."""
import argparse
import pathlib
import statistics
import sys
import time

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))
import numpy as np
import torch

from volume_segmantics_amd import _lib as L
from volume_segmantics_amd.utilities import base_data_utils as U
from volume_segmantics_amd.utilities import surface_distance as sd

REPO = pathlib.Path(__file__).resolve().parents[1]
DEV = "cuda:0"
SIDE = 512


def median_ms(fn, warmup=2, repeats=10):
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
    return statistics.median(times)


def streaming_rate():
    """bytes/s of a read-only pass over 1 GiB (tools/hbm_probe.py: torch's own sum of a bf16 tensor)"""
    x = torch.randn(1 << 29, device=DEV, dtype=torch.bfloat16)
    ms = median_ms(lambda: x.sum())
    return x.numel() * 2 / (ms * 1e-3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "surface_distances.txt"))
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--no-scipy", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("surface_probe: no GPU - nothing here is measured on a host")
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    if args.no_scipy:
        ndimage = None

    shape = (SIDE, SIDE, SIDE)
    n = SIDE ** 3
    labels = np.tile(U.numpy_from_hdf5(REPO / "tests" / "golden" / "vessels_256cube_LABELS.h5", "/data")[0], (2, 2, 2))
    vessels = torch.from_numpy(np.searchsorted(np.unique(labels), labels).astype(np.uint8)).to(DEV)
    shifted = torch.roll(vessels, shifts=(1, 1, 1), dims=(0, 1, 2)).contiguous()
    g = torch.Generator(device=DEV).manual_seed(0)
    rand_t = torch.randint(0, 4, shape, device=DEV, dtype=torch.uint8, generator=g)
    rand_p = torch.randint(0, 4, shape, device=DEV, dtype=torch.uint8, generator=g)
    lone_t = torch.zeros(shape, dtype=torch.uint8, device=DEV)
    lone_t[SIDE // 2:, :, :] = 1                                    # the truth: a half space (one plane of surface voxels)
    lone_p = torch.zeros(shape, dtype=torch.uint8, device=DEV)
    lone_p[0, 0, 0] = 1                                             # the prediction: one voxel in a corner
    cases = [("1 vessels 2x2x2 (truth) to themselves shifted by one voxel (prediction), class 1", vessels, shifted, 1),
             ("2 uniform random labels, K = 4, class 1", rand_t, rand_p, 1),
             ("3 a half space (truth) to a single-voxel class in a corner (prediction), class 1", lone_t, lone_p, 1)]

    stream = streaming_rate()
    bins = sd.histogram_bins(shape)
    masks = [torch.empty(n, dtype=torch.uint8, device=DEV) for _ in range(2)]
    counts = torch.empty(2, dtype=torch.int64, device=DEV)
    d2 = torch.empty(n, dtype=torch.int32, device=DEV)
    hist = torch.empty(bins, dtype=torch.int64, device=DEV)
    need = int(L.lib.vs_edt_workspace_bytes(*shape))
    work = torch.empty(need, dtype=torch.uint8, device=DEV)
    lines = [f"surface distances on {SIDE}^3 uint8 label volumes ({torch.cuda.get_device_name(0)}); HIP events, 2 warm-up calls, median of "
             f"{args.repeats}; one class and one direction (truth surface to predicted surface) per case; workspace {need} bytes, {bins} bins",
             f"read-only streaming rate of this box in this run (torch sum over 1 GiB, tools/hbm_probe.py): {stream / 1e12:.2f} TB/s",
             "bytes per pass, compulsory traffic: surface 2 per voxel (labels read, mask written; the neighbour rows and planes come from the "
             "caches), transform x 5 (seeds read, d2 written), y and z 8 each (d2 read and written), histogram 5 at most (mask read, d2 read "
             "where the mask is set); rate = those bytes / time, as a share of the streaming rate"]
    ok = True
    for name, truth, pred, cls in cases:
        t, p = truth.reshape(-1), pred.reshape(-1)

        def surface():
            L.check(L.lib.vs_label_surface(L.ptr(t), None, cls, *shape, L.ptr(masks[0]), L.ptr(counts[0:1]), L.stream_ptr()))

        def edt():
            L.check(L.lib.vs_edt_squared(L.ptr(masks[1]), *shape, L.ptr(d2), L.ptr(work) if need else None, need, L.stream_ptr()))

        def histogram():
            L.check(L.lib.vs_surface_distance_histogram(L.ptr(masks[0]), L.ptr(d2), n, bins, L.ptr(hist), L.stream_ptr()))

        L.check(L.lib.vs_label_surface(L.ptr(p), None, cls, *shape, L.ptr(masks[1]), L.ptr(counts[1:2]), L.stream_ptr()))
        s_ms = median_ms(surface, repeats=args.repeats)
        e_ms = median_ms(edt, repeats=args.repeats)
        h_ms = median_ms(histogram, repeats=args.repeats)
        L.check(L.lib.vs_profile_enable(1))
        for _ in range(args.repeats):
            edt()
        torch.cuda.synchronize()
        records = [r[2] for r in L.profile_read_raw()]
        L.check(L.lib.vs_profile_enable(0))
        per_call = len(records) // args.repeats
        passes = [statistics.median(records[i::per_call]) for i in range(per_call)]
        h = hist.cpu().numpy()
        surf = counts.cpu().tolist()
        same = int(h.sum()) == surf[0]
        ok &= same

        def share(nbytes, ms):
            return f"{nbytes * n / (ms * 1e-3) / 1e12:.2f} TB/s = {nbytes * n / (ms * 1e-3) / stream:.2f}"

        line = (f"case {name}: {surf[0]} truth and {surf[1]} predicted surface voxels, {100.0 * h[0] / max(surf[0], 1):.0f} % of the truth's at "
                f"d2 = 0, largest d2 {int(np.flatnonzero(h[:-1])[-1]) if h[:-1].any() else 'none'} | surface {s_ms:.3f} ms ({share(2, s_ms)}) | "
                f"transform {e_ms:.3f} ms: " + ", ".join(f"{axis} {ms:.3f} ms ({share(b, ms)})" for axis, ms, b in zip("xyz", passes, (5, 8, 8)))
                + f" | histogram {h_ms:.3f} ms ({share(5, h_ms)}) | histogram total {'equals' if same else 'DIFFERS FROM'} the surface count")
        if ndimage is not None:
            seeds = masks[1].cpu().numpy().reshape(shape) != 0
            t0 = time.perf_counter()
            ref = ndimage.distance_transform_edt(~seeds)
            host_s = time.perf_counter() - t0
            equal = bool(np.array_equal(np.rint(ref ** 2).astype(np.uint32), d2.cpu().numpy().view(np.uint32).reshape(shape)))
            ok &= equal
            line += f" | scipy distance_transform_edt on the host {host_s:.1f} s = {host_s * 1e3 / e_ms:.0f}x the transform, squared and rounded {'equal' if equal else 'DIFFERENT'}"
        lines.append(line)
        print(line, flush=True)

    text = "\n".join(lines) + "\n"
    print(text)
    out = pathlib.Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(text)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
