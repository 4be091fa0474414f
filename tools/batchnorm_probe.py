"""Measured error over bound of the BatchNorm kernels (csrc/norm.hip), per kernel form, case and quantity, on the cases and against the
float64 references of tests/batchnorm_cases.py - the figures tests/test_hip_batchnorm.py asserts to be at most 1 - and the relative
error of the convolution epilogue's variance against |mean| / std (tests/test_hip_ring_kernels.py holds the same launches to their
bound).  `python tools/batchnorm_probe.py > profiles/batchnorm.txt` on the GPU box is the record of what was measured."""
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO), str(REPO / "tests")]

import torch  # noqa: E402

import batchnorm_cases as B  # noqa: E402


def main():
    assert torch.cuda.is_available(), "the probe measures the HIP kernels: it needs the GPU"
    t0 = time.time()
    print(f"BatchNorm kernels on {torch.cuda.get_device_name(0)}, torch {torch.__version__}: measured error / bound per quantity "
          f"(sums: gamma_k(L + rpb + 2) sum|term|; y: {B.APPLY_ROUNDINGS} roundings; dx: {B.DX_ROUNDINGS} roundings; bf16: + half an ulp of the "
          f"stored value; `ulps` figures: distance in fp32 units in the last place, bound 1)")
    worst = {}

    def note(family, case, figures):
        print(f"{family:26s} {case:40s} " + ", ".join(f"{label} {r:.3g}" for label, r in figures))
        for label, r in figures:
            key = f"{family} {label.split()[-1] if 'ulps' not in label else label.split()[-2] + ' ulps'}"
            worst[key] = max(worst.get(key, 0.0), r) if r == r else float("nan")

    for case in B.TWO_SWEEP_CASES:
        note(f"two-sweep {case.family}", case.id, B.two_sweep_figures(case))
    for case in B.CHAINED_CASES:
        note("chained", case.id, B.chained_figures(case, B.chained_device(case)))
    for c in B.FOLD_C:
        for eps in (1e-5, 1e-3):
            note("vs_bn_fold", f"c={c} eps={eps:g}", B.fold_device(c, eps))
    for case in B.PARTIALS_CASES:
        note("inline apply partials", case.id, B.inline_forward_figures(case, "partials"))
    for case in B.BINS_CASES:
        note("inline apply bins", case.id, B.inline_forward_figures(case, "bins"))
    for nparts in B.FINALIZE_NPARTS:
        for c in (8, 24, 520):
            note("finalize partials", f"parts={nparts} c={c}", B.finalize_figures(nparts, c))
    for c, nparts in B.BWD_INLINE + B.BWD_FALLTHROUGH:
        for many in (False, True):
            for code in (0, 1):
                note("inline bwd" if (c, nparts) in B.BWD_INLINE else "bwd finalize + apply", f"c={c} parts={nparts} {'3wg' if many else '1wg'} {'bf16' if code else 'fp32'}",
                     B.inline_backward_figures(c, nparts, many, code, True))
    curves = {}
    for h, cin, variant in ((8, 512, 32296), (16, 256, 32296)):
        for stats in ("bins", "rows"):
            figures, curves[(h, cin, stats)] = B.ring_nonzero_mean_figures(h, cin, cin, stats, variant)
            note("conv epilogue statistics", f"{cin}to{cin}@{h} {stats}", figures)
    print("worst per family and quantity:")
    for k, v in worst.items():
        print(f"  {k:44s} {v:.3g}")
    print("the convolution epilogue's unshifted statistics against rho = |mean| / std of the output channel (float64 reference): worst relative "
          "error of var and of invstd (eps 1e-5) per band of rho, and the derived bound of var relative to var")
    for (h, cin, stats), curve in curves.items():
        for lo, hi in ((0, 0.5), (0.5, 1), (1, 2), (2, 4), (4, 8), (8, 16), (16, 32)):
            band = curve[(curve[:, 0] >= lo) & (curve[:, 0] < hi)]
            if len(band):
                print(f"  {cin}to{cin}@{h} {stats:4s} rho [{lo:g}, {hi:g}): {len(band):3d} channels, var {band[:, 1].max():.2e}, invstd {band[:, 2].max():.2e}, "
                      f"bound of var {band[:, 3].max():.2e}")
    print(f"(half a bf16 unit in the last place of y is {2.0 ** -9:.2e} to {2.0 ** -8:.2e} relative)")
    print(f"{time.time() - t0:.1f} s in all, float64 references included")
    return 0 if all(v == v and v <= 1.0 for v in worst.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
