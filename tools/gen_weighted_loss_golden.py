"""Writes tests/golden/g11_weighted_losses.npz: what the reference project's own DiceLoss(weight=..., normalization='none' | 'sigmoid')
(volume_segmantics/data/pytorch3dunet_losses.py) returns, loss and gradient in float64, on small seeded inputs.  The host tests hold
the weighted restatements of data/losses.py and of tests/class_weight_cases.py to these numbers.

    python tools/gen_weighted_loss_golden.py PATH/TO/REFERENCE_CHECKOUT [--out tests/golden/g11_weighted_losses.npz]

Runs on the CPU.  Only the two loss files of the checkout are executed, loaded by path under their own module names (the package's
__init__ pulls in the whole training stack); nothing of the checkout is copied: the fixture holds inputs, weights and results."""
import argparse
import importlib.util
import os
import sys
import types
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parent.parent
SHAPE = (2, 3, 9, 7)
WEIGHTS = {"ones": (1.0, 1.0, 1.0), "mild": (0.5, 1.0, 1.5), "steep": (0.03, 0.27, 2.7)}


def load_reference_losses(checkout: Path):
    sys.dont_write_bytecode = True
    pkg = checkout / "volume_segmantics"
    for name in ("volume_segmantics", "volume_segmantics.utilities", "volume_segmantics.data"):
        module = types.ModuleType(name)
        module.__path__ = []
        sys.modules.setdefault(name, module)
    loaded = {}
    for name, rel in (("volume_segmantics.utilities.pytorch3dunet_utils", "utilities/pytorch3dunet_utils.py"),
                      ("volume_segmantics.data.pytorch3dunet_losses", "data/pytorch3dunet_losses.py")):
        spec = importlib.util.spec_from_file_location(name, pkg / rel)
        module = importlib.util.module_from_spec(spec)
        sys.modules[name] = module
        spec.loader.exec_module(module)
        loaded[name] = module
    return loaded["volume_segmantics.data.pytorch3dunet_losses"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reference", help="path of a checkout of the reference project")
    ap.add_argument("--out", default=str(REPO / "tests" / "golden" / "g11_weighted_losses.npz"))
    args = ap.parse_args()
    os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
    losses = load_reference_losses(Path(args.reference))
    gen = torch.Generator().manual_seed(1100)
    n, k, h, w = SHAPE
    logits = (torch.randn(SHAPE, generator=gen, dtype=torch.float64) * 2.0)
    labels = torch.randint(0, k, (n, h, w), generator=gen)
    targets = torch.nn.functional.one_hot(labels, k).permute(0, 3, 1, 2).contiguous().to(torch.uint8)
    out = {"logits": logits.numpy(), "targets": targets.numpy()}
    for wname, values in WEIGHTS.items():
        weight = torch.tensor(values, dtype=torch.float64)
        out[f"{wname}__weight"] = weight.numpy()
        for norm in ("none", "sigmoid"):
            crit = losses.DiceLoss(weight=weight, normalization=norm)
            x = logits.clone().requires_grad_()
            loss = crit(x, targets)
            loss.backward()
            assert loss.dtype == torch.float64 and x.grad.dtype == torch.float64
            out[f"{wname}__{norm}__loss"], out[f"{wname}__{norm}__grad"] = loss.detach().numpy(), x.grad.numpy()
            print(f"g11 {wname} {norm}: {float(loss.detach()):.15f}")
    np.savez_compressed(args.out, **out)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
