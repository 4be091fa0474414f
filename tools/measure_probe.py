"""Times of the measurement sweep (csrc/measure.hip: vs_component_moments) on resident 512^3 label volumes with their roots already
labelled (needs a GPU), next to four yardsticks taken in the same run: the read-only streaming rate of this box by the method of
tools/hbm_probe.py; vs_component_sizes on the same roots - the same pass with one accumulator, the floor; a torch-on-device route
- ``index_add_`` of int64 per sum field and ``scatter_reduce_`` per bound over the measured voxels (the exposed faces are left out
of it: they would need six more shifted comparisons); and the host route of utilities/measurements.py (one call, roots included).
HIP events around each call, warm-up first, median of the repeats.

    python tools/measure_probe.py [--out profiles/measurements.txt] [--repeats 10] [--no-host]

Cases, the volumes of tools/components_probe.py: the vessels labels tiled 2x2x2 (connectivity 6, objects only); uniform random
labels, K = 4, under connectivity 26 with min_voxels 64 and the background measured (four giants beside crumbs that are skipped);
one solid volume with the background measured (every voxel into one row).  Exit status 1 when the kernel's sums and bounds differ
from the torch route's or its voxel counts from vs_component_sizes."""
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
from volume_segmantics_amd.utilities import components as co
from volume_segmantics_amd.utilities import measurements as me

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


def torch_route(comp, row_of_root, rows, shape):
    """the sums and bounds (fields 0 - 15) by index_add_ / scatter_reduce_ of int64, one call per field"""
    n = comp.numel()
    row = row_of_root[comp.to(torch.int64)].to(torch.int64)
    at = torch.nonzero(row >= 0).reshape(-1)
    row = row[at]
    x, line = at % shape[2], at // shape[2]
    y, z = line % shape[1], line // shape[1]
    table = torch.zeros((rows, 16), dtype=torch.int64, device=comp.device)
    for f, what in enumerate((torch.ones_like(at), z, y, x, z * z, y * y, x * x, z * y, z * x, y * x)):
        table[:, f] = torch.zeros(rows, dtype=torch.int64, device=comp.device).index_add_(0, row, what)
    for f, (what, how, start) in enumerate(((z, "amin", n), (z, "amax", -1), (y, "amin", n), (y, "amax", -1), (x, "amin", n), (x, "amax", -1))):
        table[:, 10 + f] = torch.full((rows,), start, dtype=torch.int64, device=comp.device).scatter_reduce_(0, row, what, how, include_self=True)
    return table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "measurements.txt"))
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("measure_probe: no GPU - nothing here is measured on a host")

    shape = (SIDE, SIDE, SIDE)
    n = SIDE ** 3
    vessels = np.ascontiguousarray(np.tile(U.numpy_from_hdf5(REPO / "tests" / "golden" / "vessels_256cube_LABELS.h5", "/data")[0], (2, 2, 2)))
    g = torch.Generator(device=DEV).manual_seed(0)
    cases = [("1 vessels 2x2x2 (values 0 and 255), connectivity 6, objects only", torch.from_numpy(vessels).to(DEV), 6, 1, False),
             ("2 uniform random labels, K = 4, connectivity 26, min_voxels 64, background measured",
              torch.randint(0, 4, shape, device=DEV, dtype=torch.uint8, generator=g), 26, 64, True),
             ("3 one solid volume (value 1), background measured", torch.ones(shape, dtype=torch.uint8, device=DEV), 6, 1, True)]
    stream = streaming_rate()
    lines = [f"per-component measurements on {SIDE}^3 uint8 label volumes ({torch.cuda.get_device_name(0)}); HIP events, 2 warm-up calls, median of "
             f"{args.repeats}; the roots are labelled beforehand (vs_label_components: profiles/components.txt)",
             f"read-only streaming rate of this box in this run (torch sum over 1 GiB, tools/hbm_probe.py): {stream / 1e12:.2f} TB/s",
             "bytes per voxel, compulsory traffic of the sweep: 1 (the labels; the four neighbouring rows come from the caches, ids and rows are "
             "read once per run); rate = those bytes / time, as a share of the streaming rate"]
    ok = True
    for name, labels, connectivity, min_voxels, background in cases:
        flat = labels.reshape(-1)
        comp = co.label_device(flat, shape, connectivity)
        size, touches = co.sizes_device(comp, shape)
        roots = torch.nonzero(size).reshape(-1)
        keep = size[roots] >= min_voxels
        if not background:
            keep &= flat[roots] != 0
        values, order = torch.sort(flat[roots][keep].to(torch.int64), stable=True)
        roots = roots[keep][order]
        rows = int(roots.numel())
        row_of_root = torch.full((n,), -1, dtype=torch.int32, device=DEV)
        row_of_root[roots] = torch.arange(rows, dtype=torch.int32, device=DEV)
        table = torch.empty((rows, len(me.FIELDS)), dtype=torch.int64, device=DEV)

        def sweep():
            L.check(L.lib.vs_component_moments(L.ptr(flat), L.ptr(comp), L.ptr(row_of_root), *shape, rows, L.ptr(table), L.stream_ptr()))

        def sizes():
            L.check(L.lib.vs_component_sizes(L.ptr(comp), *shape, L.ptr(size), L.ptr(touches), L.stream_ptr()))

        m_ms = median_ms(sweep, repeats=args.repeats)
        s_ms = median_ms(sizes, repeats=args.repeats)
        t_ms = median_ms(lambda: torch_route(comp, row_of_root, rows, shape), warmup=1, repeats=max(2, args.repeats // 3))
        want = torch_route(comp, row_of_root, rows, shape)
        equal = bool(torch.equal(table[:, :16], want)) and bool(torch.equal(table[:, 0], size[roots].to(torch.int64)))
        ok &= equal
        measured = int(table[:, 0].sum())
        line = (f"case {name}: {rows} rows, {measured} of {n} voxels measured, largest {int(table[:, 0].max()) if rows else 0} | sweep {m_ms:.3f} ms "
                f"({n / (m_ms * 1e-3) / 1e12:.2f} TB/s = {n / (m_ms * 1e-3) / stream:.2f}) | vs_component_sizes on the same roots {s_ms:.3f} ms "
                f"(sweep = {m_ms / s_ms:.1f}x) | torch index_add_ / scatter_reduce_ of int64, 16 fields without the faces {t_ms:.1f} ms "
                f"(= {t_ms / m_ms:.0f}x the sweep), sums and bounds {'equal' if equal else 'DIFFERENT'}")
        if not args.no_host:
            host_volume = labels.cpu().numpy()
            t0 = time.perf_counter()
            raw = me.measure_components(host_volume, connectivity, min_voxels, include_background=background, device="cpu")
            host_s = time.perf_counter() - t0
            same = np.array_equal(raw["table"], table.cpu().numpy())
            ok &= same
            line += f" | host route, roots included: {host_s:.1f} s, all 20 fields {'equal' if same else 'DIFFERENT'}"
        lines.append(line)
        print(line, flush=True)
        del comp, size, touches, row_of_root, table, want

    text = "\n".join(lines) + "\n"
    out_path = pathlib.Path(args.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(text)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
