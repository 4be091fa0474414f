"""Per-class loss weights (settings key `loss_class_weights`) in the loss kernels of csrc/loss.hip: the measured errors of every case
of tests/test_hip_class_weights.py against their bounds, and what the weights cost - each weighted forward and backward sweep through
the C ABI at the headline step's shape (32, K, 256, 256), K = 2 and 4, beside the unweighted entry point of the same build.

    python tools/class_weight_probe.py [--out profiles/class_weights.txt] [--no-errors] [--no-times]

Timing: device events around WINDOW back-to-back calls of ONE entry point, after a warm-up of the same calls; the two forms alternate,
SAMPLES windows each; reported are the median and the 10th .. 90th percentile per call, and the ratio of the medians.  The claim to
check is "no added launch, no added sweep": the weighted forward is the same two launches, the weighted backward the same one."""
import argparse
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO), str(REPO / "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

SHAPE, CLASSES = (32, 256, 256), (2, 4)
CRITERIA = ("Dice", "BCEDiceLoss", "BCELoss", "CrossEntropyLoss")
KINDS = {"BCEDiceLoss": 1, "BCELoss": 2, "CrossEntropyLoss": 3}
ALPHA, BETA, EPS = 0.75, 0.25, 1e-6
WARMUP, WINDOW, SAMPLES = 20, 50, 15
DEV = "cuda:0"


def make_calls(L, name, x, t, cw, dx, loss):
    """{(sweep, form): call} for one criterion: forward and backward, unweighted and weighted (valid null), each on its own workspace
    that a forward has filled"""
    n, k, hw = x.shape[0], x.shape[1], x.shape[2] * x.shape[3]
    p, lib = L.ptr, L.lib
    if name == "Dice":
        nbytes = lib.vs_dice_workspace(k)
        ws, wws = (torch.empty(nbytes // 4, dtype=torch.float32, device=DEV) for _ in range(2))
        calls = {("forward", "unweighted"): lambda: L.check(lib.vs_dice_loss_fwd(p(x), p(t), 0, n, k, hw, EPS, p(loss), p(ws), nbytes, None)),
                 ("forward", "weighted"): lambda: L.check(lib.vs_dice_loss_fwd_weighted(p(x), p(t), 0, None, p(cw), n, k, hw, EPS, p(loss), p(wws), nbytes, None)),
                 ("backward", "unweighted"): lambda: L.check(lib.vs_dice_loss_bwd(p(x), p(t), 0, None, n, k, hw, EPS, p(ws), p(dx), None)),
                 ("backward", "weighted"): lambda: L.check(lib.vs_dice_loss_bwd_weighted(p(x), p(t), 0, None, p(cw), None, n, k, hw, EPS, p(wws), p(dx), None))}
    else:
        kind = KINDS[name]
        nbytes, wbytes = lib.vs_seg_loss_workspace(k), lib.vs_seg_loss_weighted_workspace(k)
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=DEV)
        wws = torch.empty(wbytes // 4, dtype=torch.float32, device=DEV)
        calls = {("forward", "unweighted"): lambda: L.check(lib.vs_seg_loss_fwd(kind, p(x), p(t), 0, n, k, hw, ALPHA, BETA, EPS, p(loss), p(ws), nbytes, None)),
                 ("forward", "weighted"): lambda: L.check(lib.vs_seg_loss_fwd_weighted(kind, p(x), p(t), 0, None, p(cw), n, k, hw, ALPHA, BETA, EPS, p(loss), p(wws), wbytes, None)),
                 ("backward", "unweighted"): lambda: L.check(lib.vs_seg_loss_bwd(kind, p(x), p(t), 0, None, n, k, hw, p(ws), p(dx), None)),
                 ("backward", "weighted"): lambda: L.check(lib.vs_seg_loss_bwd_weighted(kind, p(x), p(t), 0, None, p(cw), None, n, k, hw, p(wws), p(dx), None))}
    calls[("forward", "unweighted")]()
    calls[("forward", "weighted")]()
    return calls


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


def time_lines():
    from volume_segmantics_amd import _lib as L
    n, h, w = SHAPE
    lines = [f"times: logits ({n}, K, {h}, {w}) fp32, uint8 one-hot targets, weights linspace(0.5, 1.5, K), no mask; us per call through the C ABI: "
             f"median [10th .. 90th percentile] of {SAMPLES} windows of {WINDOW} calls, the two forms alternating",
             f"{'criterion':18s} {'K':>2s} {'sweep':>8s}  {'unweighted us':>28s}  {'weighted us':>28s}  {'ratio':>6s}"]
    worst = 0.0
    for k in CLASSES:
        rng = np.random.default_rng([9200, k])
        x = torch.tensor(rng.standard_normal((n, k, h, w)).astype(np.float32)).to(DEV)
        labels = torch.tensor(rng.integers(0, k, (n, h, w)).astype(np.uint8)).to(DEV)
        t = torch.empty((n, k, h, w), dtype=torch.uint8, device=DEV)
        L.check(L.lib.vs_onehot_u8(L.ptr(labels), n, k, h * w, L.ptr(t), None))
        cw = torch.tensor(np.linspace(0.5, 1.5, k).astype(np.float32)).to(DEV)
        dx, loss = torch.empty_like(x), torch.empty((), dtype=torch.float32, device=DEV)
        for name in CRITERIA:
            calls = make_calls(L, name, x, t, cw, dx, loss)
            for sweep in ("forward", "backward"):
                fig = {form: stats(s) for form, s in alternate({form: calls[(sweep, form)] for form in ("unweighted", "weighted")}).items()}
                u, m = fig["unweighted"], fig["weighted"]
                worst = max(worst, m[0] / u[0])
                lines.append(f"{name:18s} {k:2d} {sweep:>8s}  {u[0]:9.1f} [{u[1]:7.1f} .. {u[2]:7.1f}]  {m[0]:9.1f} [{m[1]:7.1f} .. {m[2]:7.1f}]  {m[0] / u[0]:6.3f}")
    lines.append(f"largest weighted / unweighted ratio of the medians: {worst:.3f}")
    return lines


def error_lines():
    import class_weight_cases as W
    lines = ["errors: every case of tests/test_hip_class_weights.py::test_weighted_loss_and_gradient_against_the_float64_formulas, measured / bound "
             "(module route with grad_out = 1.7, C ABI with the null grad_out)", ""]
    worst = {}
    over = []
    for param in W.WEIGHTED_PARAMS:
        figures = W.weighted_figures(*param)
        lines.append(f"{W.weighted_id(param):64s} " + "  ".join(f"{label} {err:.2e}/{bound:.2e}" for label, err, bound in figures if bound > 0))
        for label, err, bound in figures:
            if bound > 0:
                worst[label] = max(worst.get(label, 0.0), err / bound)
            if not err <= bound:
                over.append((W.weighted_id(param), label, err, bound))
    lines.append("")
    lines.append("largest measured / bound per figure: " + ", ".join(f"{label} {ratio:.3f}" for label, ratio in worst.items()))
    lines.append(f"cases over their bound: {len(over)}" + "".join(f"\n  {cid} {label}: {err:.3e} of {bound:.3e}" for cid, label, err, bound in over))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "class_weights.txt"))
    ap.add_argument("--no-errors", action="store_true")
    ap.add_argument("--no-times", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe runs the HIP kernels: it needs the GPU"
    lines = [f"per-class loss weights in csrc/loss.hip on {torch.cuda.get_device_name(0)}, torch {torch.__version__}", ""]
    if not args.no_times:
        lines += time_lines() + [""]
    if not args.no_errors:
        lines += error_lines()
    text = "\n".join(lines) + "\n"
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
