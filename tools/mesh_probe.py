"""Times of the surface-mesh sweeps (csrc/mesh.hip: vs_mesh_count with its scan, vs_mesh_emit) on resident 512^3 label volumes (needs a
GPU), next to two yardsticks taken in the same run: the read-only streaming rate of this box by the method of tools/hbm_probe.py,
and the host route of utilities/meshes.py (one call), whose arrays must equal the device's.  HIP events around each call, warm-up
first, median of the repeats.

    python tools/mesh_probe.py [--out profiles/meshes.txt] [--repeats 10] [--no-host]

Cases, the volumes of tools/components_probe.py: the vessels labels tiled 2x2x2 (value 255); uniform random labels, K = 4, value 1
(nearly every cell active); one solid volume (only the border cells active).  Bytes moved: one byte per voxel read per pass (the
other three rows of voxels a row of cells needs come from the caches), 16 bytes per 64-cell chunk written by the count pass and
read by the emit pass, and the outputs - 12 bytes per vertex, 16 per quad.  Exit status 1 when an array of the device differs from
the host route's."""
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
from volume_segmantics_amd.utilities import meshes as me

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
    ap.add_argument("--out", default=str(REPO / "profiles" / "meshes.txt"))
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mesh_probe: no GPU - nothing here is measured on a host")

    shape = (SIDE, SIDE, SIDE)
    n = SIDE ** 3
    vessels = np.ascontiguousarray(np.tile(U.numpy_from_hdf5(REPO / "tests" / "golden" / "vessels_256cube_LABELS.h5", "/data")[0], (2, 2, 2)))
    g = torch.Generator(device=DEV).manual_seed(0)
    cases = [("1 vessels 2x2x2, value 255", torch.from_numpy(vessels).to(DEV), 255),
             ("2 uniform random labels, K = 4, value 1", torch.randint(0, 4, shape, device=DEV, dtype=torch.uint8, generator=g), 1),
             ("3 one solid volume, value 1", torch.ones(shape, dtype=torch.uint8, device=DEV), 1)]
    stream = streaming_rate()
    need = int(L.lib.vs_mesh_workspace_bytes(*shape))
    chunks = (SIDE + 1) * (SIDE + 1) * ((SIDE + 1 + 63) // 64)
    lines = [f"surface meshes of {SIDE}^3 uint8 label volumes, style smooth ({torch.cuda.get_device_name(0)}); HIP events, 2 warm-up calls, median of "
             f"{args.repeats}; workspace {need} bytes = {need / (SIDE + 1) ** 3:.3f} byte per cell",
             f"read-only streaming rate of this box in this run (torch sum over 1 GiB, tools/hbm_probe.py): {stream / 1e12:.2f} TB/s",
             "bytes moved: count = 1 per voxel + 16 per chunk written (the scan's passes over those 8-byte words are left out); emit = 1 per voxel + 16 "
             "per chunk read + 12 per vertex + 16 per quad written; rate = those bytes / time, as a share of the streaming rate"]
    ok = True
    for name, labels, value in cases:
        flat = labels.reshape(-1)
        work = torch.empty(need, dtype=torch.uint8, device=DEV)
        totals = torch.empty(4, dtype=torch.int64, device=DEV)

        def count():
            L.check(L.lib.vs_mesh_count(L.ptr(flat), *shape, value, L.ptr(work), need, L.ptr(totals), L.stream_ptr()))

        c_ms = median_ms(count, repeats=args.repeats)
        counts = totals.cpu().tolist()
        n_vertices, n_quads = counts[0], sum(counts[1:])
        vertices = torch.empty((n_vertices, 3), dtype=torch.float32, device=DEV)
        quads = torch.empty((n_quads, 4), dtype=torch.int32, device=DEV)

        def emit():
            L.check(L.lib.vs_mesh_emit(L.ptr(flat), *shape, value, me.STYLES["smooth"], L.ptr(work), need, L.ptr(vertices), L.ptr(quads), L.stream_ptr()))

        e_ms = median_ms(emit, repeats=args.repeats)
        c_bytes, e_bytes = n + 16 * chunks, n + 16 * chunks + 12 * n_vertices + 16 * n_quads
        line = (f"case {name}: {n_vertices} vertices, {n_quads} quads (z {counts[1]}, y {counts[2]}, x {counts[3]}) | count with its scan {c_ms:.3f} ms "
                f"({c_bytes / 1e6:.0f} MB, {c_bytes / (c_ms * 1e-3) / 1e12:.2f} TB/s = {c_bytes / (c_ms * 1e-3) / stream:.2f}) | emit {e_ms:.3f} ms "
                f"({e_bytes / 1e6:.0f} MB, {e_bytes / (e_ms * 1e-3) / 1e12:.2f} TB/s = {e_bytes / (e_ms * 1e-3) / stream:.2f}; "
                f"{n_vertices / (e_ms * 1e-3) / 1e9:.2f} G vertices/s, {n_quads / (e_ms * 1e-3) / 1e9:.2f} G quads/s)")
        if not args.no_host:
            host_volume = labels.cpu().numpy()
            t0 = time.perf_counter()
            want = me.extract_surface(host_volume, value, "smooth", device="cpu")
            host_s = time.perf_counter() - t0
            same = (want["quads_per_axis"].tolist() == counts[1:] and want["vertices"].tobytes() == vertices.cpu().numpy().tobytes()
                    and np.array_equal(want["quads"], quads.cpu().numpy()))
            ok &= same
            line += f" | host route: {host_s:.1f} s (= {host_s * 1e3 / (c_ms + e_ms):.0f}x count + emit), all arrays {'equal' if same else 'DIFFERENT'}"
            del want
        lines.append(line)
        print(line, flush=True)
        del work, vertices, quads

    text = "\n".join(lines) + "\n"
    out_path = pathlib.Path(args.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(text)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
