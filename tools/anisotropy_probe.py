"""Times of the kernels behind voxel_spacing (csrc/surface.hip: vs_edt_squared_scaled; csrc/thickness.hip: vs_thickness_centres_scaled,
_paint_scaled, _resolve_scaled) on the 512^3 vessels labels tiled 2x2x2, value 255 (needs a GPU), next to the unscaled entry points
and the read-only streaming rate of the same run (the method of tools/hbm_probe.py).  HIP events around each step, warm-up first,
median of the repeats; the transform per pass (x, y, z) from the library's own profile records.

    python tools/anisotropy_probe.py [--out profiles/anisotropy.txt] [--repeats 5] [--parent-lib libvolseg_hip.so of the parent commit]

Transform: vs_edt_squared, then vs_edt_squared_scaled under (1, 1, 1) - which must give the same bits -, (3, 1, 1) and (5, 2, 2).
Thickness under (3, 1, 1): centres (with the kept fraction), ordering the list, paint, resolve - beside the unscaled steps on the same
volume.  With --parent-lib the unscaled transform and the unscaled thickness steps of this library and of the parent's run in turns
(the side that goes first changes from round to round) on the SAME buffers, so that only the code differs, and both medians are
reported with each side's own run-to-run spread (min - max): the unscaled paths are meant to be the same code.  The file ends with
where the scaled kernels are poor, worked out from the numbers of the run.  Exit status 1 when (1, 1, 1) differs from the unscaled
transform or a property of T2 fails."""
import argparse
import ctypes
import pathlib
import statistics
import sys

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))
import numpy as np
import torch

from volume_segmantics_amd import _lib as L
from volume_segmantics_amd.utilities import base_data_utils as U
from volume_segmantics_amd.utilities import thickness as th

REPO = pathlib.Path(__file__).resolve().parents[1]
DEV = "cuda:0"
SIDE = 512
SHAPE = (SIDE, SIDE, SIDE)
UNSCALED = ("vs_edt_workspace_bytes", "vs_edt_squared", "vs_thickness_workspace_bytes", "vs_thickness_centres", "vs_thickness_paint", "vs_thickness_resolve")


def once(fn):
    """milliseconds of one fn() by HIP events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    return statistics.median(once(fn) for _ in range(repeats))


def streaming_rate():
    """bytes/s of a read-only pass over 1 GiB (tools/hbm_probe.py: torch's own sum of a bf16 tensor)"""
    x = torch.randn(1 << 29, device=DEV, dtype=torch.bfloat16)
    ms = timed(lambda: x.sum(), 2, 10)
    return x.numel() * 2 / (ms * 1e-3)


def open_library(path):
    """another build of the library with the signatures of the unscaled entry points"""
    lib = ctypes.CDLL(str(path))
    for name in UNSCALED:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = L._SIGS[name]
    return lib


def edt_call(lib, seeds, d2, work, weights=None):
    need = work.numel()
    if weights is None:
        return lambda: L.check(lib.vs_edt_squared(L.ptr(seeds), *SHAPE, L.ptr(d2), L.ptr(work) if need else None, need, L.stream_ptr()))
    return lambda: L.check(lib.vs_edt_squared_scaled(L.ptr(seeds), *SHAPE, *weights, L.ptr(d2), L.ptr(work) if need else None, need, L.stream_ptr()))


def per_pass(fn, repeats):
    """median milliseconds of the x, y and z pass from the library's profile records"""
    L.check(L.lib.vs_profile_enable(1))
    for _ in range(repeats):
        fn()
    torch.cuda.synchronize()
    records = [r[2] for r in L.profile_read_raw()]
    L.check(L.lib.vs_profile_enable(0))
    per_call = len(records) // repeats
    return [statistics.median(records[i::per_call]) for i in range(per_call)]


class Thickness:
    """the thickness steps of one library on one R, unscaled (weights None) or scaled; every step a callable without arguments"""

    def __init__(self, lib, flat, value, r, weights=None, share=None):
        self.lib, self.flat, self.value, self.r, self.w = lib, flat, value, r, weights
        self.extra = () if weights is None else tuple(weights)
        self.suffix = "" if weights is None else "_scaled"
        if share is not None:                  # another library on the buffers of `share`
            for name in ("member", "voxels", "max_r", "need", "list", "totals", "levels", "work", "t2"):
                setattr(self, name, getattr(share, name))
            return
        n = flat.numel()
        self.member = flat == value
        self.voxels = int(self.member.sum())
        self.max_r = int((r.to(torch.int64) & 0xFFFFFFFF).max())
        table = th.need_table(self.max_r) if weights is None else th.need_table_scaled(self.max_r, weights)
        self.need = torch.from_numpy(table.view(np.int32)).to(DEV)
        self.list = torch.empty(self.voxels, dtype=torch.int32, device=DEV)
        self.totals = torch.empty(2, dtype=torch.int64, device=DEV)
        self.levels = th.table_levels(SIDE, self.max_r, 1 if weights is None else weights[2] ** 2)
        self.work = torch.empty(4 * self.levels * n, dtype=torch.uint8, device=DEV)
        self.t2 = torch.zeros(n, dtype=torch.int32, device=DEV)

    def fn(self, name):
        return getattr(self.lib, name + self.suffix)

    def centres(self):
        L.check(self.fn("vs_thickness_centres")(L.ptr(self.r), *SHAPE, *self.extra, L.ptr(self.need), self.need.shape[1], L.ptr(self.list), self.voxels,
                                                L.ptr(self.totals), L.stream_ptr()))

    def order(self):
        self.count, self.rows = (int(t) for t in self.totals.cpu())
        self.ordered, self.plan = th.order_centres(self.r, self.list[:self.count], SHAPE, self.max_r, self.w or (1, 1, 1))

    def paint(self):
        for i, (begin, end, largest) in enumerate(self.plan):
            L.check(self.fn("vs_thickness_paint")(L.ptr(self.r), *SHAPE, *self.extra, self.ordered.data_ptr() + 4 * begin, end - begin, largest, self.max_r,
                                                  L.ptr(self.work), self.work.numel(), int(i == 0), L.stream_ptr()))

    def resolve(self):
        L.check(self.fn("vs_thickness_resolve")(L.ptr(self.flat), *SHAPE, *self.extra, self.value, self.max_r, L.ptr(self.work), self.work.numel(),
                                                L.ptr(self.t2), L.stream_ptr()))

    def holds(self):
        m = self.member
        return bool((self.t2[m].to(torch.int64) >= self.r[m].to(torch.int64)).all()) and int(self.t2.max()) == self.max_r and not bool(self.t2[~m].any())


def thickness_line(name, t, repeats, stream, edt_ms, figures):
    n = t.flat.numel()
    centres_ms = timed(t.centres, 1, repeats)
    order_ms = timed(t.order, 1, repeats)
    zero_ms = timed(lambda: t.work.zero_(), 1, repeats)
    paint_ms = timed(t.paint, 1, repeats)
    resolve_ms = timed(t.resolve, 0, 1)                # in place: once, on the table the last paint left
    ok = t.holds()
    paint_only = max(paint_ms - zero_ms, 1e-6)
    figures[name] = dict(centres_ms=centres_ms, paint_ms=paint_ms, rate=t.rows / (paint_only * 1e-3), kept=t.count / t.voxels, rows=t.rows)
    return (f"thickness {name}: largest R {t.max_r}, table rows of {t.need.shape[1]} entries | {t.count} centres kept of {t.voxels} voxels "
            f"({100.0 * t.count / t.voxels:.1f} %), {t.rows} row spans in {len(t.plan)} launch(es) | transform {edt_ms:.2f} ms | centres {centres_ms:.2f} ms "
            f"({4 * n / (centres_ms * 1e-3) / stream:.2f} of the streaming rate for one read of R) | ordering the list (torch) {order_ms:.2f} ms | paint "
            f"{paint_ms:.2f} ms of which zeroing the table {zero_ms:.2f} ms: {t.rows / (paint_only * 1e-3) / 1e9:.2f} G row spans/s | resolve {resolve_ms:.2f} ms, "
            f"{t.levels} levels | T2 >= R on M, max T2 = max R, T2 = 0 off M: {'hold' if ok else 'FAIL'}"), ok


def spread(samples):
    return f"{statistics.median(samples):.3f} ms (min {min(samples):.3f} - max {max(samples):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "anisotropy.txt"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("anisotropy_probe: no GPU - nothing here is measured on a host")

    vessels = np.ascontiguousarray(np.tile(U.numpy_from_hdf5(REPO / "tests" / "golden" / "vessels_256cube_LABELS.h5", "/data")[0], (2, 2, 2)))
    flat = torch.from_numpy(vessels).to(DEV).reshape(-1)
    n, value = flat.numel(), 255
    seeds = (flat != value).to(torch.uint8)
    stream = streaming_rate()
    lines = [f"voxel_spacing kernels on the {SIDE}^3 vessels labels tiled 2x2x2, value {value} ({torch.cuda.get_device_name(0)}); HIP events, 1 warm-up call, "
             f"median of {args.repeats}; the transform's passes from the library's profile records",
             f"read-only streaming rate of this box in this run (torch sum over 1 GiB, tools/hbm_probe.py): {stream / 1e12:.2f} TB/s"]
    work = torch.empty(int(L.lib.vs_edt_workspace_bytes(*SHAPE)), dtype=torch.uint8, device=DEV)
    ok, maps, edt_ms, pass_ms, figures = True, {}, {}, {}, {}
    for weights in (None, (1, 1, 1), (3, 1, 1), (5, 2, 2)):
        d2 = torch.empty(n, dtype=torch.int32, device=DEV)
        call = edt_call(L.lib, seeds, d2, work, weights)
        edt_ms[weights] = timed(call, 1, args.repeats)
        passes = pass_ms[weights] = per_pass(call, args.repeats)
        maps[weights] = d2
        name = "vs_edt_squared" if weights is None else f"vs_edt_squared_scaled {weights}"
        lines.append(f"transform {name}: {edt_ms[weights]:.3f} ms = {edt_ms[weights] / edt_ms[None]:.2f} x vs_edt_squared | "
                     + ", ".join(f"{axis} {ms:.3f} ms ({b * n / (ms * 1e-3) / stream:.2f} of the streaming rate)" for axis, ms, b in zip("xyz", passes, (5, 8, 8)))
                     + f" | largest value {int((d2.to(torch.int64) & 0xFFFFFFFF).max())}")
        print(lines[-1], flush=True)
    same = bool(torch.equal(maps[None], maps[(1, 1, 1)]))
    ok &= same
    lines.append(f"weights (1, 1, 1) through the scaled entry: {'the bits of vs_edt_squared' if same else 'DIFFERENT from vs_edt_squared'}")

    for name, weights in (("unscaled", None), ("under (3, 1, 1)", (3, 1, 1))):
        t = Thickness(L.lib, flat, value, maps[weights], weights)
        line, good = thickness_line(name, t, args.repeats, stream, edt_ms[weights], figures)
        ok &= good
        lines.append(line)
        print(line, flush=True)
        del t
        torch.cuda.empty_cache()
    del maps[(1, 1, 1)], maps[(3, 1, 1)], maps[(5, 2, 2)]
    torch.cuda.empty_cache()

    if args.parent_lib:
        parent = open_library(args.parent_lib)
        r = maps[None]
        mine = Thickness(L.lib, flat, value, r)
        sides = {"this commit": mine, "the parent": Thickness(parent, flat, value, r, share=mine)}
        d2 = torch.empty(n, dtype=torch.int32, device=DEV)
        calls = {"this commit": edt_call(L.lib, seeds, d2, work), "the parent": edt_call(parent, seeds, d2, work)}
        samples = {side: {step: [] for step in ("transform", "centres", "paint", "resolve")} for side in sides}
        for side, t in sides.items():                     # warm-up, and the list each side paints
            calls[side]()
            t.centres()
            t.order()
            t.paint()
        maps_of, equal = {}, True
        for i in range(2 * args.repeats):
            for side in (list(sides) if i % 2 == 0 else list(sides)[::-1]):       # in turns; who goes first changes every round
                t = sides[side]
                samples[side]["transform"].append(once(calls[side]))
                samples[side]["centres"].append(once(t.centres))
                samples[side]["paint"].append(once(t.paint))
                samples[side]["resolve"].append(once(t.resolve))
                if i == 0:
                    maps_of[side] = t.t2.clone()
        equal = bool(torch.equal(maps_of["this commit"], maps_of["the parent"]))
        ok &= equal
        lines.append(f"unscaled entry points, this commit's library and the parent's in turns on the same buffers, {2 * args.repeats} rounds, the first side "
                     f"changing every round; T2 {'equal' if equal else 'DIFFERENT'}")
        for step in ("transform", "centres", "paint", "resolve"):
            lines.append(f"  {step}: " + " | ".join(f"{side} {spread(samples[side][step])}" for side in sides))
            print(lines[-1], flush=True)
    a, b = figures["unscaled"], figures["under (3, 1, 1)"]
    lines += ["where the scaled kernels are poor (from the numbers above):",
              f"  transform: the x pass and the passes along an axis of weight 1 cost what they cost unscaled ((3, 1, 1): y {pass_ms[(3, 1, 1)][1]:.3f} ms against "
              f"{pass_ms[None][1]:.3f} ms); only a coarse axis gains, for its search ends after fewer steps (z {pass_ms[(3, 1, 1)][2]:.3f} ms against "
              f"{pass_ms[None][2]:.3f} ms).  The y and z passes stay at 0.1 - 0.2 of the streaming rate, as they are unscaled: the outward search, not memory, "
              f"is the cost.  Weights with a common scale such as (5, 2, 2) gain nothing over (3, 1, 1): the stop rule sees only the ratio.",
              f"  scaled (1, 1, 1) against vs_edt_squared: {edt_ms[(1, 1, 1)] / edt_ms[None]:.3f} x - the one difference in code is the multiplication by q in the inner loop of the column passes; "
              f"an isotropic spacing never takes this path.",
              f"  centres: {b['centres_ms']:.2f} ms against {a['centres_ms']:.2f} ms unscaled - seven table rows read per voxel instead of three, and the sweep was "
              f"already far below the streaming rate.  {100 * b['kept']:.1f} % of the voxels stay centres ({100 * a['kept']:.1f} % unscaled).",
              f"  paint: {b['rate'] / 1e9:.1f} G row spans/s against {a['rate'] / 1e9:.1f} unscaled: a ball under (3, 1, 1) has a third of the planes, so a batch of 64 "
              f"centres has fewer rows to spread over its waves, and every row adds an integer division by q (supposed causes: not profiled); the paint is still shorter in all "
              f"({b['paint_ms']:.1f} ms against {a['paint_ms']:.1f} ms) because there are fewer row spans ({b['rows']} against {a['rows']}).",
              "  resolve: the same kernel and the same level count here; a coarse x axis would lower the level count, a fine x axis under coarse z and y raises "
              "max R / qx and with it the table's size - the table is K full volumes whatever the weights.",
              "  histograms under a spacing: one masked maximum (torch, an int64 temporary of the volume) per histogram before the kernel; not timed here."]
    out_path = pathlib.Path(args.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text("\n".join(lines) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
