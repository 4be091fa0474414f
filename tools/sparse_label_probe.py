"""What the validity mask of sparse labels (settings key `ignore_label`) costs in the loss kernels of csrc/loss.hip: forward + backward
of every criterion through the C ABI at the headline step's shape (32, K, 256, 256), K = 2 and 4, unmasked entry points against the
_masked ones with every 8th row valid, and the streaming rate of a device copy in the same run.

    python tools/sparse_label_probe.py [--out profiles/sparse_labels.txt] [--parent-lib PATH/libvolseg_hip.so]

Timing: device events around WINDOW back-to-back forward + backward pairs, after a warm-up of the same calls; the two forms alternate,
SAMPLES windows each; reported are the median and the 10th .. 90th percentile per pair.  --parent-lib: a build of the parent commit's
library.  The unmasked times are then taken in fresh child processes (VOLSEG_HIP_LIB selects the library), this tree's and the
parent's alternating, each child under its own time limit, and a difference counts only beyond the spread of this tree's own rounds."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import tempfile
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO), str(REPO / "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

SHAPE, CLASSES = (32, 256, 256), (2, 4)
CRITERIA = ("Dice", "BCEDiceLoss", "BCELoss", "CrossEntropyLoss", "GeneralizedDiceLoss")
KINDS = {"BCEDiceLoss": 1, "BCELoss": 2, "CrossEntropyLoss": 3, "GeneralizedDiceLoss": 4}
ALPHA, BETA, EPS = 0.75, 0.25, 1e-6
WARMUP, WINDOW, SAMPLES = 20, 50, 15
CHILD_LIMIT, ROUNDS = 240, 3
DEV = "cuda:0"


class Library:
    """the entry points this probe times, bound straight from a libvolseg_hip.so (the package's own binding wants every symbol of
    this tree's header, which a build of the parent commit does not have)"""
    I, P, F, I64, SZ = ctypes.c_int, ctypes.c_void_p, ctypes.c_float, ctypes.c_int64, ctypes.c_size_t
    SIGS = {"vs_dice_workspace": (SZ, [I]), "vs_seg_loss_workspace": (SZ, [I]), "vs_seg_loss_masked_workspace": (SZ, [I]),
            "vs_onehot_u8": (I, [P, I, I, I64, P, P]),
            "vs_dice_loss_fwd": (I, [P, P, I, I, I, I64, F, P, P, SZ, P]), "vs_dice_loss_bwd": (I, [P, P, I, P, I, I, I64, F, P, P, P]),
            "vs_seg_loss_fwd": (I, [I, P, P, I, I, I, I64, F, F, F, P, P, SZ, P]), "vs_seg_loss_bwd": (I, [I, P, P, I, P, I, I, I64, P, P, P]),
            "vs_dice_loss_fwd_masked": (I, [P, P, I, P, I, I, I64, F, P, P, SZ, P]),
            "vs_dice_loss_bwd_masked": (I, [P, P, I, P, P, I, I, I64, F, P, P, P]),
            "vs_seg_loss_fwd_masked": (I, [I, P, P, I, P, I, I, I64, F, F, F, P, P, SZ, P]),
            "vs_seg_loss_bwd_masked": (I, [I, P, P, I, P, P, I, I, I64, P, P, P])}

    def __init__(self, path=None):
        path = path or os.environ.get("VOLSEG_HIP_LIB") or REPO / "volume-segmantics_amd" / "lib" / "libvolseg_hip.so"
        self.lib = ctypes.CDLL(str(path))
        for name, (restype, argtypes) in self.SIGS.items():
            if hasattr(self.lib, name):      # (the masked ones are absent from a parent build)
                fn = getattr(self.lib, name)
                fn.restype, fn.argtypes = restype, argtypes

    @staticmethod
    def ptr(tensor):
        return None if tensor is None else ctypes.c_void_p(tensor.data_ptr())

    @staticmethod
    def check(rc):
        if rc != 0:
            raise RuntimeError(f"libvolseg_hip call failed with {rc}")


def make_call(L, name, x, t, valid, dx, loss):
    """one forward + backward of a criterion; valid None: the unmasked entry points"""
    n, k, hw = x.shape[0], x.shape[1], x.shape[2] * x.shape[3]
    p = L.ptr
    if name == "Dice":
        nbytes = L.lib.vs_dice_workspace(k)
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=DEV)
        if valid is None:
            return lambda: (L.check(L.lib.vs_dice_loss_fwd(p(x), p(t), 0, n, k, hw, EPS, p(loss), p(ws), nbytes, None)),
                            L.check(L.lib.vs_dice_loss_bwd(p(x), p(t), 0, None, n, k, hw, EPS, p(ws), p(dx), None)))
        return lambda: (L.check(L.lib.vs_dice_loss_fwd_masked(p(x), p(t), 0, p(valid), n, k, hw, EPS, p(loss), p(ws), nbytes, None)),
                        L.check(L.lib.vs_dice_loss_bwd_masked(p(x), p(t), 0, p(valid), None, n, k, hw, EPS, p(ws), p(dx), None)))
    kind = KINDS[name]
    nbytes = L.lib.vs_seg_loss_workspace(k) if valid is None else L.lib.vs_seg_loss_masked_workspace(k)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=DEV)
    if valid is None:
        return lambda: (L.check(L.lib.vs_seg_loss_fwd(kind, p(x), p(t), 0, n, k, hw, ALPHA, BETA, EPS, p(loss), p(ws), nbytes, None)),
                        L.check(L.lib.vs_seg_loss_bwd(kind, p(x), p(t), 0, None, n, k, hw, p(ws), p(dx), None)))
    return lambda: (L.check(L.lib.vs_seg_loss_fwd_masked(kind, p(x), p(t), 0, p(valid), n, k, hw, ALPHA, BETA, EPS, p(loss), p(ws), nbytes, None)),
                    L.check(L.lib.vs_seg_loss_bwd_masked(kind, p(x), p(t), 0, p(valid), None, n, k, hw, p(ws), p(dx), None)))


def window_us(call):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(WINDOW):
        call()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1000.0 / WINDOW


def alternate(calls):
    """{label: [us per call, SAMPLES windows]}, the labels taking turns"""
    for call in calls.values():
        for _ in range(WARMUP):
            call()
    torch.cuda.synchronize()
    out = {label: [] for label in calls}
    for _ in range(SAMPLES):
        for label, call in calls.items():
            out[label].append(window_us(call))
    return out


def stats(samples):
    return float(np.median(samples)), float(np.percentile(samples, 10)), float(np.percentile(samples, 90))


def inputs(k):
    n, h, w = SHAPE
    rng = np.random.default_rng([9000, k])
    x = torch.tensor(rng.standard_normal((n, k, h, w)).astype(np.float32)).to(DEV)
    labels = torch.tensor(rng.integers(0, k, (n, h, w)).astype(np.uint8)).to(DEV)
    labels[:, [r for r in range(h) if r % 8]] = 255
    return x, labels


def measure(masked: bool):
    """[(criterion, K, {label: (median, p10, p90)})] plus the copy rate"""
    L = Library()
    rows = []
    for k in CLASSES:
        x, labels = inputs(k)
        n, hw = x.shape[0], x.shape[2] * x.shape[3]
        t = torch.empty((n, k) + tuple(x.shape[2:]), dtype=torch.uint8, device=DEV)
        L.check(L.lib.vs_onehot_u8(L.ptr(labels), n, k, hw, L.ptr(t), None))
        valid = (labels != 255).to(torch.uint8) if masked else None
        dx, loss = torch.empty_like(x), torch.empty((), dtype=torch.float32, device=DEV)
        for name in CRITERIA:
            calls = {"unmasked": make_call(L, name, x, t, None, dx, loss)}
            if masked:
                calls["masked"] = make_call(L, name, x, t, valid, dx, loss)
            rows.append((name, k, {label: stats(s) for label, s in alternate(calls).items()}))
    src = torch.empty(SHAPE[0] * 4 * SHAPE[1] * SHAPE[2], dtype=torch.float32, device=DEV)
    dst = torch.empty_like(src)
    copy = stats(alternate({"copy": lambda: dst.copy_(src)})["copy"])
    return rows, (copy, 2 * src.numel() * 4)


def bytes_moved(name, k, masked):
    """HBM bytes one forward + backward must move at least: the reduction reads logits (4) and uint8 targets (1) per element, the
    gradient sweep reads both again and writes 4; the mask adds one byte per pixel and sweep (the K class planes of a pixel share
    it).  What a masked sweep may skip - the logits and targets of ignored pixels in the scalar kernels - is not subtracted."""
    n, h, w = SHAPE
    elems = n * k * h * w
    return elems * (5 + 9) + (2 * n * h * w if masked else 0)


def child(out_path):
    rows, _copy = measure(masked=False)
    Path(out_path).write_text(json.dumps([[name, k, figures["unmasked"]] for name, k, figures in rows]))
    return 0


def against_parent(parent_lib, lines):
    """the unmasked entry points, this tree's library and the parent's in alternating fresh processes"""
    medians = {"this tree": [], "parent": []}
    for r in range(ROUNDS):
        for label, lib in (("this tree", None), ("parent", parent_lib)):
            env = dict(os.environ)
            if lib:
                env["VOLSEG_HIP_LIB"] = str(Path(lib).resolve())
            else:
                env.pop("VOLSEG_HIP_LIB", None)
            with tempfile.TemporaryDirectory() as tmp:
                out = Path(tmp) / "unmasked.json"
                done = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--child", str(out)], env=env, timeout=CHILD_LIMIT)
                if done.returncode:
                    raise RuntimeError(f"child for {label} ended with {done.returncode}")
                medians[label].append({(name, k): fig[0] for name, k, fig in json.loads(out.read_text())})
    lines.append("")
    lines.append(f"unmasked entry points, this tree's library against a build of the parent commit: {ROUNDS} fresh processes each, alternating;")
    lines.append("median us per forward + backward of each process, then (parent - this tree) of the medians over the processes")
    moved = False
    for key in medians["this tree"][0]:
        mine, theirs = [m[key] for m in medians["this tree"]], [m[key] for m in medians["parent"]]
        spread = max(max(mine) - min(mine), max(theirs) - min(theirs))
        diff = float(np.median(theirs) - np.median(mine))
        verdict = "within the spread" if abs(diff) <= spread else ("this tree FASTER" if diff > 0 else "this tree SLOWER")
        moved |= diff < -spread
        lines.append(f"  {key[0]:20s} K={key[1]}  this tree {' '.join(f'{v:7.1f}' for v in mine)}   parent {' '.join(f'{v:7.1f}' for v in theirs)}"
                     f"   diff {diff:+6.1f} us, spread {spread:5.1f} us: {verdict}")
    lines.append("templating the kernels on MASKED " + ("MOVED an unmasked time beyond the spread (see above)" if moved else
                                                         "did not move the unmasked times beyond the run's own spread"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "sparse_labels.txt"))
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe times the HIP kernels: it needs the GPU"
    if args.child:
        return child(args.child)
    rows, (copy, copy_bytes) = measure(masked=True)
    rate = copy_bytes / (copy[0] * 1e-6) / 1e9
    n, h, w = SHAPE
    lines = [f"sparse labels: cost of the validity mask in csrc/loss.hip on {torch.cuda.get_device_name(0)}, torch {torch.__version__}",
             f"logits ({n}, K, {h}, {w}) fp32, uint8 one-hot targets, every 8th row valid ({100 / 8:.1f} % of the pixels); forward + backward "
             f"through the C ABI, us per pair: median [10th .. 90th percentile] of {SAMPLES} windows of {WINDOW} pairs, the two forms alternating",
             f"streaming rate of the same run: device copy of {copy_bytes / 2**20:.0f} MiB read + written in {copy[0]:.1f} us "
             f"[{copy[1]:.1f} .. {copy[2]:.1f}] = {rate:.0f} GB/s", ""]
    lines.append(f"{'criterion':20s} {'K':>2s}  {'unmasked us':>28s}  {'masked us':>28s}  {'ratio':>6s}  {'GB/s unmasked':>13s}  {'GB/s masked':>11s}  "
                 f"{'bytes ratio':>11s}")
    for name, k, fig in rows:
        u, m = fig["unmasked"], fig["masked"]
        bu, bm = bytes_moved(name, k, False), bytes_moved(name, k, True)
        lines.append(f"{name:20s} {k:2d}  {u[0]:9.1f} [{u[1]:7.1f} .. {u[2]:7.1f}]  {m[0]:9.1f} [{m[1]:7.1f} .. {m[2]:7.1f}]  {m[0] / u[0]:6.3f}  "
                     f"{bu / (u[0] * 1e-6) / 1e9:13.0f}  {bm / (m[0] * 1e-6) / 1e9:11.0f}  {bm / bu:11.3f}")
    if args.parent_lib:
        against_parent(args.parent_lib, lines)
    text = "\n".join(lines) + "\n"
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
