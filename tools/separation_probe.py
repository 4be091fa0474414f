"""Times of the separation stages (csrc/separate.hip) and of the object form of the measurement sweep (csrc/measure.hip:
vs_object_moments) on resident 512^3 label volumes (needs a GPU), every time next to the read-only streaming rate of this box measured
in the same run by the method of tools/hbm_probe.py.  HIP events around each call, one warm-up, median of the repeats; the merge is
host code and is timed by the wall clock.

    python tools/separation_probe.py [--out profiles/separation.txt] [--repeats 3] [--cases 1,2,3,4,5] [--no-host]

Cases: 1 a synthetic packing of overlapping balls (value 1); 2 the vessels labels tiled 2x2x2 (value 255); 3 one solid slab (value 1),
the plateau worst case of the basin pass; 4 and 5 uniform random labels, K = 4 (value 1) - debris, which the bound on the pair rows
(measure_separate_max_pairs, default 5 000 000) is there for: the rows are recorded, and whether the default refuses them.
Connectivity 26 (case 5: 6), depth 1.  Per case: vs_edt_squared (the floor every route pays), vs_separate_parents,
vs_separate_basins, vs_separate_pair_count, vs_separate_pairs, the host merge, vs_separate_relabel, then vs_object_moments on the
separated labelling against vs_component_moments on the component labelling of the same volume.  The host route runs on a 128^3
crop of each case and its integers are compared with the device route's on the same crop.  Exit status 1 when they differ."""
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
from volume_segmantics_amd.utilities import separation as sp
from volume_segmantics_amd.utilities import surface_distance as sd

REPO = pathlib.Path(__file__).resolve().parents[1]
DEV = "cuda:0"
SIDE = 512
DEPTH = 1.0


def median_ms(fn, setup=None, warmup=1, repeats=3):
    times = []
    for i in range(warmup + repeats):
        state = setup() if setup else None
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(state) if setup else fn()
        e1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            times.append(e0.elapsed_time(e1))
    return statistics.median(times)


def streaming_rate():
    """bytes/s of a read-only pass over 1 GiB (tools/hbm_probe.py: torch's own sum of a bf16 tensor)"""
    x = torch.randn(1 << 29, device=DEV, dtype=torch.bfloat16)
    ms = median_ms(lambda: x.sum(), repeats=10)
    return x.numel() * 2 / (ms * 1e-3)


def ball_packing(side, balls=420, seed=0):
    """overlapping balls of radius side / 16 .. side / 10 at random centres, value 1"""
    rng = np.random.default_rng(seed)
    vol = torch.zeros((side, side, side), dtype=torch.uint8, device=DEV)
    axis = torch.arange(side, device=DEV)
    for _ in range(balls):
        radius = int(rng.integers(side // 16, side // 10 + 1))
        c = rng.integers(0, side, 3)
        lo, hi = np.maximum(c - radius, 0), np.minimum(c + radius + 1, side)
        z, y, x = (axis[lo[k]:hi[k]] - int(c[k]) for k in range(3))
        inside = (z * z)[:, None, None] + (y * y)[None, :, None] + (x * x)[None, None, :] <= radius * radius
        vol[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]][inside] = 1
    return vol


def moments_rows(flat, ids, shape, min_voxels=1):
    """the row of every root of a labelling by member ids: the objects of every non-zero value, by value, then root"""
    size, _ = co.sizes_device(ids, shape)
    roots = torch.nonzero(size).reshape(-1)
    keep = (size[roots] >= min_voxels) & (flat[roots] != 0)
    _, order = torch.sort(flat[roots][keep].to(torch.int64), stable=True)
    roots = roots[keep][order]
    row_of_root = torch.full((flat.numel(),), -1, dtype=torch.int32, device=DEV)
    row_of_root[roots] = torch.arange(roots.numel(), dtype=torch.int32, device=DEV)
    return row_of_root, int(roots.numel())


def probe_case(name, labels, value, connectivity, stream, repeats, lines):
    """the stages of one value on one resident volume; returns the separated labelling (or None where the value was refused)"""
    shape = tuple(labels.shape)
    flat = labels.reshape(-1)
    n = flat.numel()
    share = lambda bytes_, ms: bytes_ / (ms * 1e-3) / stream          # noqa: E731
    seeds = (flat != value).to(torch.uint8)
    r = torch.empty(n, dtype=torch.int32, device=DEV)
    work = torch.empty(int(L.lib.vs_edt_workspace_bytes(*shape)), dtype=torch.uint8, device=DEV)
    edt_ms = median_ms(lambda: sd.edt_device(seeds, shape, r, work), repeats=repeats)
    del seeds, work
    parent = torch.empty(n, dtype=torch.int32, device=DEV)

    def parents():
        L.check(L.lib.vs_separate_parents(L.ptr(r), *shape, connectivity, L.ptr(parent), L.stream_ptr()))

    parents_ms = median_ms(parents, repeats=repeats)
    basin = torch.empty_like(parent)

    def basins(_):
        L.check(L.lib.vs_separate_basins(L.ptr(basin), *shape, L.stream_ptr()))

    basins_ms = median_ms(basins, setup=lambda: basin.copy_(parent), repeats=repeats)
    del parent
    count_ms = median_ms(lambda: sp.pair_count_device(basin, shape, connectivity), repeats=repeats)
    count = sp.pair_count_device(basin, shape, connectivity)
    peaks = torch.nonzero(basin == torch.arange(n, dtype=torch.int32, device=DEV)).reshape(-1)
    voxels = int((flat == value).sum())
    slots = sp.table_slots(count, int(peaks.numel()))
    head = (f"case {name}: value {value}, {voxels} of {n} voxels, {int(peaks.numel())} basins, {count} adjacent voxel pairs in different basins, table of "
            f"{slots} slots | vs_edt_squared {edt_ms:.2f} ms | parents {parents_ms:.2f} ms ({share(8 * n, parents_ms):.2f} of streaming for 8 B/voxel) | "
            f"basins {basins_ms:.2f} ms ({share(8 * n, basins_ms):.2f}) | pair_count {count_ms:.2f} ms ({share(4 * n, count_ms):.2f} for 4 B/voxel)")
    keys = torch.empty(slots, dtype=torch.int64, device=DEV)
    saddle = torch.empty(slots, dtype=torch.int32, device=DEV)
    faces = torch.empty((slots, 3), dtype=torch.int32, device=DEV)
    used = torch.empty(2, dtype=torch.int64, device=DEV)

    def pairs():
        L.check(L.lib.vs_separate_pairs(L.ptr(r), L.ptr(basin), *shape, connectivity, L.ptr(keys), L.ptr(saddle), L.ptr(faces), slots, L.ptr(used),
                                        L.stream_ptr()))

    pairs_ms = median_ms(pairs, repeats=repeats)
    rows = int(used[0])
    head += f" | pairs {pairs_ms:.2f} ms ({share(8 * n, pairs_ms):.2f} for 8 B/voxel; memsets of the table included), {rows} rows"
    del keys, saddle, faces
    if rows > sp.DEFAULT_MAX_PAIRS:
        try:
            sp.separate_objects(labels, values=[value], connectivity=connectivity, depth=DEPTH)
            head += " | NOT REFUSED at the default bound"
            refused = False
        except ValueError as e:
            head += f" | refused at the default bound: {e}"
            refused = True
        lines.append(head)
        print(head, flush=True)
        return None, refused
    head += f" (at or below the default bound of {sp.DEFAULT_MAX_PAIRS}: not refused)"
    table = sp.pairs_device(r, basin, shape, connectivity, slots)
    peak_r = r[peaks].cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    t0 = time.perf_counter()
    rep, merges = sp.merge_basins(peaks.cpu().numpy(), peak_r, table["a"], table["b"], table["saddle"], DEPTH)
    merge_s = time.perf_counter() - t0
    set_of_peak = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    set_of_peak[peaks] = torch.from_numpy(rep.astype(np.int32)).to(DEV)
    comp = co.label_device(flat, shape, connectivity)
    objects = comp.clone()
    relabel_ms = median_ms(lambda: sp.relabel_device(basin, set_of_peak, shape, objects), repeats=repeats)
    del basin, set_of_peak, r
    head += (f" | host merge {merge_s:.3f} s, {merges} merges, {int(peaks.numel()) - merges} objects | relabel {relabel_ms:.2f} ms "
             f"({share(16 * n, relabel_ms):.2f} for 16 B/voxel)")

    rows_c, count_c = moments_rows(flat, comp, shape)
    rows_o, count_o = moments_rows(flat, objects, shape)
    table_c = torch.empty((count_c, len(me.FIELDS)), dtype=torch.int64, device=DEV)
    table_o = torch.empty((count_o, len(me.FIELDS)), dtype=torch.int64, device=DEV)
    by_value = median_ms(lambda: L.check(L.lib.vs_component_moments(L.ptr(flat), L.ptr(comp), L.ptr(rows_c), *shape, count_c, L.ptr(table_c), L.stream_ptr())),
                         repeats=repeats)
    by_id_c = median_ms(lambda: L.check(L.lib.vs_object_moments(L.ptr(comp), L.ptr(rows_c), *shape, count_c, L.ptr(table_o[:count_c]), L.stream_ptr())),
                        repeats=repeats)
    same = bool(torch.equal(table_o[:count_c], table_c))
    by_id_o = median_ms(lambda: L.check(L.lib.vs_object_moments(L.ptr(objects), L.ptr(rows_o), *shape, count_o, L.ptr(table_o), L.stream_ptr())),
                        repeats=repeats)
    head += (f" | vs_component_moments on the {count_c} components {by_value:.2f} ms; vs_object_moments on the same labelling {by_id_c:.2f} ms "
             f"(= {by_id_c / by_value:.1f}x, {share(4 * n, by_id_c):.2f} of streaming for 4 B/voxel), tables {'equal' if same else 'DIFFERENT'}; on the {count_o} "
             f"separated objects {by_id_o:.2f} ms")
    lines.append(head)
    print(head, flush=True)
    return objects, same


def host_parity(name, labels, value, connectivity, lines):
    """the host route on the 128^3 crop at the volume's centre, against the device route on the same crop"""
    lo = SIDE // 2 - 64
    crop = labels[lo:lo + 128, lo:lo + 128, lo:lo + 128].contiguous()
    t0 = time.perf_counter()
    try:
        want = sp.separate_objects(crop.cpu().numpy(), values=[value], connectivity=connectivity, depth=DEPTH, device="cpu")
    except ValueError as e:
        line = f"case {name}, 128^3 crop, host route: refused ({e})"
        lines.append(line)
        print(line, flush=True)
        return True
    host_s = time.perf_counter() - t0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = sp.separate_objects(crop, values=[value], connectivity=connectivity, depth=DEPTH)
    device_s = time.perf_counter() - t0
    same = np.array_equal(got["objects"], want["objects"]) and got["report"] == want["report"] and \
        all(np.array_equal(got["contacts"][k], want["contacts"][k]) for k in want["contacts"])
    line = (f"case {name}, 128^3 crop: host route {host_s:.2f} s, device route (upload, components, distance map, merge and download included) "
            f"{device_s:.3f} s, {want['report'][str(value)]['objects']} objects from {want['report'][str(value)]['basins']} basins, "
            f"objects, report and contacts {'equal' if same else 'DIFFERENT'}")
    lines.append(line)
    print(line, flush=True)
    return same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "separation.txt"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cases", default="1,2,3,4,5")
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("separation_probe: no GPU - nothing here is measured on a host")
    wanted = {int(c) for c in args.cases.split(",")}
    shape = (SIDE, SIDE, SIDE)

    def vessels():
        return torch.from_numpy(np.ascontiguousarray(np.tile(U.numpy_from_hdf5(REPO / "tests" / "golden" / "vessels_256cube_LABELS.h5", "/data")[0], (2, 2, 2)))).to(DEV)

    def slab():
        vol = torch.zeros(shape, dtype=torch.uint8, device=DEV)
        vol[SIDE // 4:3 * SIDE // 4, 1:SIDE - 1, 1:SIDE - 1] = 1
        return vol

    def random_labels():
        return torch.randint(0, 4, shape, device=DEV, dtype=torch.uint8, generator=torch.Generator(device=DEV).manual_seed(0))

    cases = {1: ("1 packing of 420 overlapping balls (radius 32 .. 51), connectivity 26", lambda: ball_packing(SIDE), 1, 26),
             2: ("2 vessels 2x2x2, connectivity 26", vessels, 255, 26),
             3: (f"3 one solid slab {SIDE // 2} x {SIDE - 2} x {SIDE - 2}, connectivity 26", slab, 1, 26),
             4: ("4 uniform random labels, K = 4, connectivity 26", random_labels, 1, 26),
             5: ("5 uniform random labels, K = 4, connectivity 6", random_labels, 1, 6)}
    stream = streaming_rate()
    lines = [f"separation of touching objects on {SIDE}^3 uint8 label volumes ({torch.cuda.get_device_name(0)}), depth {DEPTH}; HIP "
             f"events, 1 warm-up call, median of {args.repeats}",
             f"read-only streaming rate of this box in this run (torch sum over 1 GiB, tools/hbm_probe.py): {stream / 1e12:.2f} TB/s; a share is the bytes "
             f"named beside it (the stage's compulsory traffic) / time / that rate"]
    ok = True
    for number in sorted(wanted):
        name, build, value, connectivity = cases[number]
        labels = build()
        _, fine = probe_case(name, labels, value, connectivity, stream, args.repeats, lines)
        ok &= bool(fine)
        if not args.no_host:
            ok &= host_parity(name, labels, value, connectivity, lines)
        del labels
        torch.cuda.empty_cache()
    out_path = pathlib.Path(args.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text("\n".join(lines) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
