"""Times of the overlap-table sweeps (csrc/overlap.hip: vs_overlap_runs, vs_overlap_table) on resident 512^3 root volumes that are
already labelled (needs a GPU), next to yardsticks taken in the same run: the read-only streaming rate of this box by the method of
tools/hbm_probe.py; vs_component_sizes on the same roots - the same kind of pass with one accumulator per component, the floor;
the ``torch.unique`` route over one 64-bit key per voxel (object_scores.overlap_table_unique's device part), the baseline; and the
host route (``np.unique`` over the same keys, the keys' construction included).  HIP events around each call, warm-up first, median
of the repeats.  The table sweep is timed as the Python layer calls it - the initialisation of a table of ``slots`` entries, the
launch and the read-back of ``used`` included - with the initialisation's share (two fills of the same size) measured beside it.

    python tools/overlap_probe.py [--out profiles/object_scores.txt] [--repeats 10] [--no-host]

Cases, the volumes of tools/components_probe.py: the vessels labels tiled 2x2x2 against themselves shifted by one voxel along x with
plane y = 128, plane z = 96 and the corner [:64, :64, :64] cleared (connectivity 6); two independent volumes of uniform random
labels, K = 4, under connectivity 6 (tens of millions of components, nearly every voxel its own run); one solid volume against
itself.  Exit status 1 when the tables of the routes differ or the table sweep does not beat the ``torch.unique`` route on a volume."""
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
from volume_segmantics_amd.utilities import object_scores as obs

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


def unique_route(a, b):
    return torch.unique((a.to(torch.int64) << 32) | b.to(torch.int64), return_counts=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "object_scores.txt"))
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("overlap_probe: no GPU - nothing here is measured on a host")

    shape = (SIDE, SIDE, SIDE)
    n = SIDE ** 3
    truth = np.ascontiguousarray(np.tile(U.numpy_from_hdf5(REPO / "tests" / "golden" / "vessels_256cube_LABELS.h5", "/data")[0] > 0, (2, 2, 2))).astype(np.uint8)
    pred = np.zeros_like(truth)
    pred[:, :, 1:] = truth[:, :, :-1]
    pred[:, 128, :] = 0
    pred[96] = 0
    pred[:64, :64, :64] = 0
    g = torch.Generator(device=DEV).manual_seed(0)
    solid = torch.ones(shape, dtype=torch.uint8, device=DEV)
    cases = [("1 vessels 2x2x2 against themselves shifted and cut, connectivity 6", torch.from_numpy(truth).to(DEV), torch.from_numpy(pred).to(DEV)),
             ("2 two volumes of uniform random labels, K = 4, connectivity 6", torch.randint(0, 4, shape, device=DEV, dtype=torch.uint8, generator=g),
              torch.randint(0, 4, shape, device=DEV, dtype=torch.uint8, generator=g)),
             ("3 one solid volume against itself", solid, solid)]
    del truth, pred
    stream = streaming_rate()
    lines = [f"overlap table of two labellings of {SIDE}^3 voxels ({torch.cuda.get_device_name(0)}); HIP events, 2 warm-up calls, median of "
             f"{args.repeats}; both volumes are labelled beforehand (vs_label_components: profiles/components.txt)",
             f"read-only streaming rate of this box in this run (torch sum over 1 GiB, tools/hbm_probe.py): {stream / 1e12:.2f} TB/s",
             "bytes per voxel, compulsory traffic of either sweep: 8 (two int32 roots; 9 with a skip mask, none here); rate = those bytes / time, "
             "as a share of the streaming rate.  The table sweep's time includes the initialisation of its 16 bytes per slot and the read-back of `used`"]
    ok = True
    for name, la, lb in cases:
        a, b = co.label_device(la.reshape(-1), shape, 6), co.label_device(lb.reshape(-1), shape, 6)
        size = torch.empty(n, dtype=torch.int32, device=DEV)
        touches = torch.empty(n, dtype=torch.uint8, device=DEV)
        runs_out = torch.empty(1, dtype=torch.int64, device=DEV)

        def runs_sweep():
            L.check(L.lib.vs_overlap_runs(L.ptr(a), L.ptr(b), None, n, SIDE, L.ptr(runs_out), L.stream_ptr()))

        def sizes():
            L.check(L.lib.vs_component_sizes(L.ptr(a), *shape, L.ptr(size), L.ptr(touches), L.stream_ptr()))

        r_ms = median_ms(runs_sweep, repeats=args.repeats)
        runs = int(runs_out.item())
        slots = obs.table_slots(runs)
        keys = torch.empty(slots, dtype=torch.int64, device=DEV)
        counts = torch.empty(slots, dtype=torch.int64, device=DEV)
        used = torch.empty(2, dtype=torch.int64, device=DEV)

        def table_sweep():
            L.check(L.lib.vs_overlap_table(L.ptr(a), L.ptr(b), None, n, SIDE, L.ptr(keys), L.ptr(counts), slots, L.ptr(used), L.stream_ptr()))

        def memsets():
            keys.fill_(-1)
            counts.zero_()

        t_ms = median_ms(table_sweep, repeats=args.repeats)
        m_ms = median_ms(memsets, repeats=args.repeats)
        s_ms = median_ms(sizes, repeats=args.repeats)
        del keys, counts
        whole_ms = median_ms(lambda: obs.table_device_sorted(a, b, None, SIDE), warmup=1, repeats=max(2, args.repeats // 3))
        u_ms = median_ms(lambda: unique_route(a, b), warmup=1, repeats=max(2, args.repeats // 3))
        table = obs.table_device(a, b, None, SIDE)
        want_keys, want_counts = unique_route(a, b)
        want = obs.split_keys(want_keys.cpu().numpy().view(np.uint64), want_counts.cpu().numpy())
        del want_keys, want_counts
        equal = all(np.array_equal(x, y) for x, y in zip(table, want))
        ok &= equal and t_ms < u_ms                                      # the table sweep has to beat the torch.unique route on every volume
        share =lambda ms: 8.0 * n / (ms * 1e-3) / stream                # noqa: E731
        line = (f"case {name}: {runs} runs, {len(table[0])} table rows, {slots} slots | runs sweep {r_ms:.3f} ms ({8.0 * n / (r_ms * 1e-3) / 1e12:.2f} TB/s = "
                f"{share(r_ms):.2f} of streaming) | table sweep {t_ms:.3f} ms ({8.0 * n / (t_ms * 1e-3) / 1e12:.2f} TB/s = {share(t_ms):.2f}; two fills of its size "
                f"{m_ms:.3f} ms) | vs_component_sizes on the same roots {s_ms:.3f} ms (table sweep = {t_ms / s_ms:.1f}x) | device route to the sorted table on the device - runs, "
                f"table, compaction, sort {whole_ms:.2f} ms | torch.unique over {n} int64 keys, sorted table on the device {u_ms:.2f} ms (= {u_ms / t_ms:.1f}x "
                f"the table sweep, {u_ms / whole_ms:.2f}x the whole route), tables {'equal' if equal else 'DIFFERENT'}")
        if not args.no_host:
            ha, hb = a.cpu().numpy(), b.cpu().numpy()
            t0 = time.perf_counter()
            host = obs.table_host(ha, hb, None)
            host_s = time.perf_counter() - t0
            same = all(np.array_equal(x, y) for x, y in zip(table, host))
            ok &= same
            line += f" | host route (np.unique): {host_s:.1f} s, table {'equal' if same else 'DIFFERENT'}"
            del ha, hb, host
        lines.append(line)
        print(line, flush=True)
        del a, b, size, touches, table, want
        torch.cuda.empty_cache()

    text = "\n".join(lines) + "\n"
    out_path = pathlib.Path(args.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(text)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
