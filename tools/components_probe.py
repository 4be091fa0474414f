"""Times of the connected-component kernels (csrc/components.hip: the three launches of vs_label_components, vs_component_sizes,
vs_component_largest, vs_components_apply) on 512^3 label volumes, per connectivity, next to the read-only streaming rate of this box
measured in the same run by the method of tools/hbm_probe.py and - where scipy imports - to scipy.ndimage.label on the host for the
same volume, one call per label value (needs a GPU).  HIP events around each call, warm-up first, median of the repeats; the launches
of the labelling are timed by the library's own profile records (tiles, seams, flatten in launch order).  Also the cost of uploading
the uint8 volume, which the prediction manager pays before it cleans.

    python tools/components_probe.py [--out profiles/components.txt] [--repeats 10] [--no-scipy]

Cases: the vessels labels tiled 2x2x2; uniform random labels, K = 4 (very many tiny components); one solid volume (a single
component: the worst case for same-address size counting).  Exit status 1 when the sizes do not add up to the volume or the
device's components (count and sorted sizes per value) differ from scipy's."""
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


def device_table(labels, size):
    """{value: sorted sizes} from the device's size array"""
    roots = torch.nonzero(size).reshape(-1)
    values, sizes = labels[roots].cpu().numpy(), size[roots].cpu().numpy()
    return {int(v): np.sort(sizes[values == v]) for v in np.unique(values)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "components.txt"))
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--no-scipy", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("components_probe: no GPU - nothing here is measured on a host")
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    if args.no_scipy:
        ndimage = None

    shape = (SIDE, SIDE, SIDE)
    n = SIDE ** 3
    vessels = np.ascontiguousarray(np.tile(U.numpy_from_hdf5(REPO / "tests" / "golden" / "vessels_256cube_LABELS.h5", "/data")[0], (2, 2, 2)))
    g = torch.Generator(device=DEV).manual_seed(0)
    cases = [("1 vessels 2x2x2 (values 0 and 255)", torch.from_numpy(vessels).to(DEV)),
             ("2 uniform random labels, K = 4", torch.randint(0, 4, shape, device=DEV, dtype=torch.uint8, generator=g)),
             ("3 one solid volume (value 1)", torch.ones(shape, dtype=torch.uint8, device=DEV))]

    stream = streaming_rate()
    t0 = time.perf_counter()
    uploaded = torch.from_numpy(vessels).to(DEV)
    torch.cuda.synchronize()
    upload_ms = (time.perf_counter() - t0) * 1e3
    del uploaded
    need = int(L.lib.vs_components_workspace_bytes(*shape))
    comp = torch.empty(n, dtype=torch.int32, device=DEV)
    size = torch.empty(n, dtype=torch.int32, device=DEV)
    touches = torch.empty(n, dtype=torch.uint8, device=DEV)
    out = torch.empty(n, dtype=torch.uint8, device=DEV)
    work = torch.empty(need, dtype=torch.uint8, device=DEV)
    keys = torch.empty(256, dtype=torch.int64, device=DEV)
    counts = torch.empty(4, dtype=torch.int64, device=DEV)
    min_size = torch.full((256,), 100, dtype=torch.int32, device=DEV)
    keep_root = torch.full((256,), -1, dtype=torch.int32, device=DEV)
    lines = [f"connected components on {SIDE}^3 uint8 label volumes ({torch.cuda.get_device_name(0)}); HIP events, 2 warm-up calls, median of "
             f"{args.repeats}; workspace {need} bytes (one int32 per {co.TILE_Z} x {co.TILE_Y} x {co.TILE_X} tile)",
             f"read-only streaming rate of this box in this run (torch sum over 1 GiB, tools/hbm_probe.py): {stream / 1e12:.2f} TB/s",
             f"uploading the {n >> 20} MiB uint8 volume from pageable host memory (what the prediction manager pays before cleaning): {upload_ms:.1f} ms",
             "bytes per voxel, compulsory traffic: labelling 13 (tiles: labels read 1, ids written 4; flatten: ids read and written 8; the seams "
             "read only the faces of tiles that are not of one value), sizes 9 (ids read 4, size and touches zeroed 5), largest 4 (sizes read), "
             "apply 6 (labels 1, ids 4, cleaned volume 1; min_object_size 100 everywhere, fill_holes 1000); rate = those bytes / time, as a share "
             "of the streaming rate"]
    ok = True
    for name, labels in cases:
        flat = labels.reshape(-1)
        host = labels.cpu().numpy() if ndimage is not None else None
        for connectivity in (6, 18, 26):
            def label():
                L.check(L.lib.vs_label_components(L.ptr(flat), *shape, connectivity, L.ptr(comp), L.ptr(work), need, L.stream_ptr()))

            def sizes():
                L.check(L.lib.vs_component_sizes(L.ptr(comp), *shape, L.ptr(size), L.ptr(touches), L.stream_ptr()))

            def largest():
                L.check(L.lib.vs_component_largest(L.ptr(flat), L.ptr(size), n, L.ptr(keys), L.stream_ptr()))

            def apply():
                L.check(L.lib.vs_components_apply(L.ptr(flat), L.ptr(comp), L.ptr(size), L.ptr(touches), L.ptr(min_size), L.ptr(keep_root), 0, 1000, n,
                                                  L.ptr(out), L.ptr(counts), L.stream_ptr()))

            l_ms = median_ms(label, repeats=args.repeats)
            s_ms = median_ms(sizes, repeats=args.repeats)
            g_ms = median_ms(largest, repeats=args.repeats)
            a_ms = median_ms(apply, repeats=args.repeats)
            L.check(L.lib.vs_profile_enable(1))
            for _ in range(args.repeats):
                label()
            torch.cuda.synchronize()
            records = [r[2] for r in L.profile_read_raw()]
            L.check(L.lib.vs_profile_enable(0))
            per_call = len(records) // args.repeats
            launches = [statistics.median(records[i::per_call]) for i in range(per_call)]
            table = device_table(flat, size)
            total = int(sum(int(s.sum()) for s in table.values()))
            ok &= total == n

            def share(nbytes, ms):
                return f"{nbytes * n / (ms * 1e-3) / 1e12:.2f} TB/s = {nbytes * n / (ms * 1e-3) / stream:.2f}"

            line = (f"case {name}, connectivity {connectivity}: " + ", ".join(f"value {v}: {len(s)} components, largest {int(s[-1])}" for v, s in table.items())
                    + f" | labelling {l_ms:.3f} ms ({share(13, l_ms)}): " + ", ".join(f"{what} {ms:.3f} ms" for what, ms in zip(("tiles", "seams", "flatten"), launches))
                    + f" | sizes {s_ms:.3f} ms ({share(9, s_ms)}) | largest {g_ms:.3f} ms ({share(4, g_ms)}) | apply {a_ms:.3f} ms ({share(6, a_ms)}), "
                    + "cleared {} components / {} voxels, filled {} holes / {} voxels".format(*counts.cpu().tolist())
                    + f" | sizes {'add up to' if total == n else 'DO NOT ADD UP TO'} the volume")
            if ndimage is not None:
                structure = ndimage.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[connectivity])
                host_s, equal = 0.0, True
                for value in np.unique(host):
                    t0 = time.perf_counter()
                    labelled, count = ndimage.label(host == value, structure=structure, output=np.int32)
                    host_s += time.perf_counter() - t0
                    theirs = np.sort(np.bincount(labelled.reshape(-1), minlength=count + 1)[1:])
                    equal &= int(value) in table and np.array_equal(theirs, table[int(value)])
                ok &= equal
                device_ms = l_ms + s_ms
                line += (f" | scipy.ndimage.label on the host, one call per value: {host_s:.1f} s = {host_s * 1e3 / device_ms:.0f}x labelling + sizes, "
                         f"component counts and sorted sizes per value {'equal' if equal else 'DIFFERENT'}")
            lines.append(line)
            print(line, flush=True)

    text = "\n".join(lines) + "\n"
    print(text)
    out_path = pathlib.Path(args.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(text)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
