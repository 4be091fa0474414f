"""Times of the local-thickness kernels (csrc/thickness.hip: vs_thickness_centres, vs_thickness_paint, vs_thickness_resolve) on resident
512^3 label volumes (needs a GPU), next to the yardsticks of the same run: the read-only streaming rate of this box by the method of
tools/hbm_probe.py, and vs_edt_squared on the same seeds - the floor, for R has to be made whatever paints the balls.  HIP events
around each step, warm-up first, median of the repeats.  Putting the centre list in order (torch) is timed as its own step.

    python tools/thickness_probe.py [--out profiles/thickness.txt] [--repeats 3] [--cases 1,2,3] [--no-host]

Cases: the vessels labels tiled 2x2x2 (value 255: radii up to 48, a quarter of the voxels stay centres); uniform random labels, K = 4,
value 1 (R of 1 - 2, nearly every voxel a centre, balls of one to nine rows); one ball of radius 200 (spans hundreds long, and - the
lattice test is borderline inside one large ball - more than half of its voxels stay centres).  Per
case: centres kept out of voxels, row spans (the rows of every kept ball's bounding square inside the volume - what a lane is
spent on) and their rate over the paint time, the launches, the levels and bytes of the table.  The host route of
utilities/thickness.py runs on a 128^3 crop of case 1 and must give the device's integers there; its time for 512^3 is that time
x 64, an extrapolation by volume, and is labelled so.  Exit status 1 when integers differ or a property of T2 fails."""
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
from volume_segmantics_amd.utilities import thickness as th

REPO = pathlib.Path(__file__).resolve().parents[1]
DEV = "cuda:0"
SIDE = 512
HEAVY_ROWS = 2 * 10 ** 10


def timed(fn, warmup, repeats):
    """median milliseconds of fn() by HIP events"""
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
    ms = timed(lambda: x.sum(), 2, 10)
    return x.numel() * 2 / (ms * 1e-3)


def ball_volume(radius):
    zi, yi, xi = np.ogrid[:SIDE, :SIDE, :SIDE]
    c = SIDE // 2
    return (((zi - c) ** 2 + (yi - c) ** 2 + (xi - c) ** 2) <= radius * radius).astype(np.uint8)


def run_case(name, labels, value, repeats, stream):
    shape = (SIDE, SIDE, SIDE)
    flat = labels.reshape(-1)
    n = flat.numel()
    member = flat == value
    voxels = int(member.sum())
    seeds = (~member).to(torch.uint8)
    r = torch.empty(n, dtype=torch.int32, device=DEV)
    edt_work = torch.empty(int(L.lib.vs_edt_workspace_bytes(*shape)), dtype=torch.uint8, device=DEV)
    edt_ms = timed(lambda: sd.edt_device(seeds, shape, r, edt_work), 1, repeats)
    max_r = int(r.max())
    need = torch.from_numpy(th.need_table(max_r).view(np.int32)).to(DEV)
    centres = torch.empty(voxels, dtype=torch.int32, device=DEV)
    totals = torch.empty(2, dtype=torch.int64, device=DEV)

    def find():
        L.check(L.lib.vs_thickness_centres(L.ptr(r), *shape, L.ptr(need), need.shape[1], L.ptr(centres), voxels, L.ptr(totals), L.stream_ptr()))

    centres_ms = timed(find, 1, repeats)
    count, rows = (int(t) for t in totals.cpu())
    kept = {}

    def order():
        kept["centres"], kept["plan"] = th.order_centres(r, centres[:count], shape, max_r)

    sort_ms = timed(order, 1, repeats)
    plan = kept["plan"]
    levels = th.table_levels(SIDE, max_r)
    work_bytes = int(L.lib.vs_thickness_workspace_bytes(*shape, max_r))
    work = torch.empty(work_bytes, dtype=torch.uint8, device=DEV)
    t2 = torch.zeros(n, dtype=torch.int32, device=DEV)
    ordered = kept["centres"]

    def paint():
        for i, (begin, end, largest) in enumerate(plan):
            L.check(L.lib.vs_thickness_paint(L.ptr(r), *shape, ordered.data_ptr() + 4 * begin, end - begin, largest, max_r, L.ptr(work), work_bytes,
                                             int(i == 0), L.stream_ptr()))

    def resolve():
        L.check(L.lib.vs_thickness_resolve(L.ptr(flat), *shape, value, max_r, L.ptr(work), work_bytes, L.ptr(t2), L.stream_ptr()))

    zero_ms = timed(lambda: work.zero_(), 1, repeats)
    heavy = rows > HEAVY_ROWS                        # a case of many seconds is painted once, cold
    paint_ms = timed(paint, 0 if heavy else 1, 1 if heavy else repeats)      # includes zeroing the table
    by_r = ""
    if not heavy:                                    # the other order: by R alone, largest first
        radii, by = torch.sort(torch.index_select(r, 0, centres[:count]).to(torch.int64) & 0xFFFFFFFF, descending=True)
        distinct, counts = torch.unique_consecutive(radii, return_counts=True)
        mine, ordered, plan = (ordered, plan), centres[:count][by].contiguous(), th.launch_plan(distinct.cpu().numpy(), counts.cpu().numpy(), shape, th.LAUNCH_ROWS)
        by_r = f" (the list sorted by R alone: {timed(paint, 1, repeats):.2f} ms in {len(plan)} launches)"
        (ordered, plan) = mine
        paint()
    resolve_ms = timed(resolve, 0, 1)                # in place: timed once, on the table the last paint left
    bins = sd.histogram_bins(shape)
    hist = torch.empty(bins, dtype=torch.int64, device=DEV)
    mask = member.to(torch.uint8)
    hist_ms = timed(lambda: L.check(L.lib.vs_surface_distance_histogram(L.ptr(mask), L.ptr(t2), n, bins, L.ptr(hist), L.stream_ptr())), 1, repeats)
    ok = bool((t2[member] >= r[member]).all()) and int(t2.max()) == max_r and not bool(t2[~member].any()) and int(hist.sum()) == voxels
    total_ms = edt_ms + centres_ms + sort_ms + paint_ms + resolve_ms + hist_ms
    paint_only = max(paint_ms - zero_ms, 1e-6)
    line = (f"case {name}: {voxels} of {n} voxels, largest R {max_r} | {count} centres kept ({100.0 * count / voxels:.1f} % of the voxels), {rows} row spans "
            f"in {len(plan)} launch(es){', painted once without a warm-up' if heavy else ''} | vs_edt_squared {edt_ms:.2f} ms (the floor) | centres {centres_ms:.2f} ms ({4 * n / (centres_ms * 1e-3) / stream:.2f} of the "
            f"streaming rate for one read of R) | ordering the list (torch) {sort_ms:.2f} ms | paint {paint_ms:.2f} ms of which zeroing the table {zero_ms:.2f} ms{by_r}: "
            f"{rows / (paint_only * 1e-3) / 1e9:.2f} G row spans/s | resolve {resolve_ms:.2f} ms, {levels} levels ({4 * n * (3 * (levels - 1) + 1) / (resolve_ms * 1e-3) / stream:.2f} "
            f"of the streaming rate for 3 (levels - 1) + 1 volumes) | histogram {hist_ms:.2f} ms | all steps {total_ms:.1f} ms = {total_ms / edt_ms:.1f} x the floor | "
            f"table {levels} x {4 * n} = {work_bytes} bytes | T2 >= R on M, max T2 = max R, T2 = 0 off M, histogram total: {'hold' if ok else 'FAIL'}")
    return line, ok, rows / (paint_only * 1e-3), t2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "thickness.txt"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cases", default="1,2,3")
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("thickness_probe: no GPU - nothing here is measured on a host")

    shape = (SIDE, SIDE, SIDE)
    vessels = np.ascontiguousarray(np.tile(U.numpy_from_hdf5(REPO / "tests" / "golden" / "vessels_256cube_LABELS.h5", "/data")[0], (2, 2, 2)))
    g = torch.Generator(device=DEV).manual_seed(0)
    cases = [("1 vessels 2x2x2, value 255", lambda: torch.from_numpy(vessels).to(DEV), 255),
             ("2 uniform random labels, K = 4, value 1", lambda: torch.randint(0, 4, shape, device=DEV, dtype=torch.uint8, generator=g), 1),
             ("3 one ball of radius 200, value 1", lambda: torch.from_numpy(ball_volume(200)).to(DEV), 1)]
    stream = streaming_rate()
    lines = [f"local thickness on {SIDE}^3 uint8 label volumes ({torch.cuda.get_device_name(0)}); HIP events, 1 warm-up call, median of {args.repeats} "
             f"(the in-place resolve: one call on a freshly painted table)",
             f"read-only streaming rate of this box in this run (torch sum over 1 GiB, tools/hbm_probe.py): {stream / 1e12:.2f} TB/s",
             "a row span = one row (dz, dy) of a kept ball's bounding square inside the volume: one lane's work - a load or two and at most two 32-bit "
             "atomic maxima; the rate is row spans over the paint time without the table's memset"]
    ok, rate_vessels, first = True, None, None
    wanted = {c.strip() for c in args.cases.split(",")}
    for name, make, value in cases:
        if name.split()[0] not in wanted:
            continue
        labels = make()
        line, good, rate, t2 = run_case(name, labels, value, args.repeats, stream)
        ok &= good
        lines.append(line)
        print(line, flush=True)
        if name.startswith("1 "):
            rate_vessels, first = rate, t2.cpu().numpy().view(np.uint32).reshape(shape)
        del labels, t2
        torch.cuda.empty_cache()
    if rate_vessels is not None:
        lines.append(f"thickness_max_work: the vessels rate x 60 s = {rate_vessels * 60:.3g} row spans; utilities/thickness.py DEFAULT_MAX_WORK = {th.DEFAULT_MAX_WORK:.3g}")
    if not args.no_host and first is not None:
        crop = np.ascontiguousarray(vessels[:128, :128, :128])
        t0 = time.perf_counter()
        host = th.local_thickness_squared(crop, 255, device="cpu")
        host_s = time.perf_counter() - t0
        device = th.local_thickness_squared(crop, 255, device=DEV)
        same = np.array_equal(host, device)
        k = int(np.floor(2.0 * np.sqrt(float(host.max())))) + 1      # deep inside the crop the whole volume's map is the crop's (tests/test_hip_thickness.py)
        deep = np.array_equal(host[k:128 - k, k:128 - k, k:128 - k], first[k:128 - k, k:128 - k, k:128 - k])
        ok &= same and deep
        lines.append(f"host route (NumPy, utilities/thickness.py) on the 128^3 corner crop of case 1: {host_s:.1f} s, integers {'equal' if same else 'DIFFERENT'} to the "
                     f"device route's on the crop, and {'equal' if deep else 'DIFFERENT'} to case 1's map further than {k} voxels from the crop's faces; x 64 by "
                     f"volume = {host_s * 64 / 60:.0f} min for 512^3 - an extrapolation, not a measurement")
        print(lines[-1], flush=True)
    out_path = pathlib.Path(args.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text("\n".join(lines) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
