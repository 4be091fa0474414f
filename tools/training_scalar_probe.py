"""Measured error over bound of the training step's small kernels (csrc/loss.hip, csrc/optim.hip), per kernel and case, on the cases
and against the float64 references of tests/training_scalar_cases.py - the figures tests/test_hip_training_scalars.py asserts to be
at most 1.  `python tools/training_scalar_probe.py > profiles/training_scalars.txt` on the GPU box is the record of what was measured."""
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO), str(REPO / "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import training_scalar_cases as T  # noqa: E402


def ratio(err, bound):
    return 0.0 if err == 0 else (float("inf") if bound == 0 else err / bound)


def main():
    assert torch.cuda.is_available(), "the probe measures the HIP kernels: it needs the GPU"
    t0 = time.time()
    print(f"training scalar kernels on {torch.cuda.get_device_name(0)}, torch {torch.__version__}: measured error / bound "
          f"(bounds: loss {T.LOSS_BOUND:g} max(1, |ref|), gradient {T.GRAD_BOUND:g} max|ref|, MeanIoU {T.IOU_BOUND:g}, "
          f"moments {T.MOMENT_BOUND:g} relative, update {T.UPDATE_BOUND:g} |update| + {T.UPDATE_ULPS:g} ulp(p))")
    worst = {}

    def note(kernel, case, figures):
        line = ", ".join(f"{label} {ratio(err, bound):.3f}" for label, err, bound in figures)
        print(f"{kernel:22s} {case:44s} {line}")
        worst[kernel] = max(worst.get(kernel, 0.0), max(ratio(err, bound) for _, err, bound in figures))

    for case, name in T.LOSS_PARAMS:
        note("vs_dice_loss" if name == "Dice" else f"vs_seg_loss {name}", case.id, T.loss_figures(case, name))
    for which, (tdtype, offsets) in T.MISALIGNED.items():
        case = T.Case("misaligned", 3, tdtype=tdtype)
        logits, targets = T.inputs(case)
        for name in T.CRITERIA:
            loss, grad = T.abi_loss(name, logits, targets, None, offsets)
            note("vs_dice_loss" if name == "Dice" else f"vs_seg_loss {name}", f"misaligned {which}",
                 T.loss_errors(loss, grad, *T.reference(case, name)))
    for shape in T.IOU_SHAPES:
        for classes in T.IOU_CLASSES:
            for tdtype in ("uint8", "float32"):
                note("vs_mean_iou", f"{shape}-k{classes}-{tdtype}", T.iou_figures(shape, classes, tdtype))
    for shape in T.ONEHOT_SHAPES:
        for classes in T.ONEHOT_CLASSES:
            labels = T.onehot_labels(shape, classes)
            wrong = int((T.onehot_device(labels, classes).cpu() != T.onehot_reference(labels, classes)).sum())
            note("vs_onehot_u8", f"{shape}-k{classes}", [("bytes that differ", float(wrong), 0.0)])
    for n in T.ADAMW_SIZES:
        for step, figures, changed in T.adamw_run(n):
            note("vs_adamw_step", f"n={n} step {step}", [(label, r, 1.0) for label, r in figures] + [("masked elements changed", float(changed), 0.0)])
    print("worst per kernel: " + "; ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    print(f"{time.time() - t0:.1f} s in all, float64 references on the CPU included")
    return 0 if all(np.isfinite(v) and v <= 1.0 for v in worst.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
