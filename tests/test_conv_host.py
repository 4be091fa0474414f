"""The cases, reference and bound of tests/conv_cases.py without a GPU: the table against a hand-written list of the instantiations
launch_tile builds and against the library's own plan queries (host logic), the float64 reference against an independent float64
evaluation, and the bound against fp32 torch on the CPU - an honest fp32 convolution rounded to the stored type meets it on every
case, three seeded mutations of that computation exceed it, and for the 16-bit types it is nowhere looser than hip_helpers.tol."""
import pytest
import torch

import conv_cases as CC
from hip_helpers import lib

# launch_tile's instantiations without normalise-on-load, (BN, PT, NW, taps, stride, dilation), written out from csrc/conv_igemm.hip
TILE_TUPLES = [
    (64, 2, 4, 9, 1, 1), (32, 2, 4, 9, 1, 1), (16, 2, 4, 9, 1, 1), (64, 2, 4, 1, 1, 1), (32, 2, 4, 1, 1, 1), (16, 2, 4, 1, 1, 1),    # 128-pixel tiles
    (64, 1, 4, 9, 1, 1), (32, 1, 4, 9, 1, 1), (16, 1, 4, 9, 1, 1), (64, 1, 4, 1, 1, 1), (32, 1, 4, 1, 1, 1), (16, 1, 4, 1, 1, 1),    # 64-pixel tiles
    (64, 2, 8, 9, 1, 1), (32, 2, 8, 9, 1, 1), (16, 2, 8, 9, 1, 1), (64, 2, 8, 1, 1, 1), (32, 2, 8, 1, 1, 1), (16, 2, 8, 1, 1, 1),    # 8 waves
    (64, 1, 4, 9, 2, 1), (32, 1, 4, 9, 2, 1), (16, 1, 4, 9, 2, 1), (64, 1, 4, 1, 2, 1), (32, 1, 4, 1, 2, 1), (16, 1, 4, 1, 2, 1),    # stride 2
    (64, 2, 4, 9, 2, 1),                                                                                                            # 8 x 16 stride-2 tiles
    (64, 2, 4, 9, 1, 2), (32, 2, 4, 9, 1, 2), (64, 1, 4, 9, 1, 2), (32, 1, 4, 9, 1, 2),                                              # dilation 2
    (64, 2, 4, 9, 1, 4), (32, 2, 4, 9, 1, 4), (64, 1, 4, 9, 1, 4), (32, 1, 4, 9, 1, 4),                                              # dilation 4
]
# (instantiation, dtypes it is built for)
OTHER = [(("ring", 1), (1,)), (("ring", 2), (1,)), (("ring", 3), (1,)), (("stream", 64), (1, 2)), (("stream", 32), (1, 2)),
         (("direct",), (0, 1, 2)), (("direct-up0",), (0, 1, 2)), (("head",), (0, 1, 2))]

ALL = CC.CASES + CC.REJECTED


def test_table_has_one_row_per_instantiation_and_dtype():
    assert len(TILE_TUPLES) == 33 and len(set(TILE_TUPLES)) == 33
    rows = [(c.inst, c.code) for c in CC.CASES if c.inst is not None]
    want = [(t, code) for t in TILE_TUPLES for code in (0, 1, 2)] + [(t, code) for t, codes in OTHER for code in codes]
    assert sorted(rows, key=repr) == sorted(want, key=repr)
    assert len({c.id for c in ALL}) == len(ALL)
    forms = {c.family: set() for c in CC.CASES}
    for c in CC.CASES:
        forms[c.family] |= {f for f in ("up0", "c1", "affine", "bias", "residual", "relu", "pool0", "split_c") if getattr(c, f)}
        forms[c.family] |= {"stuffed"} if c.up0 == 2 else set()
    assert forms["tile"] >= {"up0", "c1", "stuffed", "affine", "bias", "residual", "relu", "pool0", "split_c"}
    assert forms["ring"] >= {"up0", "c1", "stuffed", "affine", "bias", "residual", "relu", "pool0", "split_c"}
    assert forms["direct"] >= {"up0", "affine", "bias", "relu", "pool0"}           # (no residual, concat, stuffing or split in direct_ok)
    assert forms["stream"] >= {"up0", "c1", "affine", "residual", "relu"}


@pytest.mark.parametrize("case", ALL, ids=lambda c: c.id)
def test_plan_code_of_the_table_is_what_the_library_selects(case):
    L = lib()
    before = {k: L.lib.vs_get_option(k.encode()) for k, _ in case.options}
    code, rows = CC.queried(L, case)
    assert code == case.plan, f"{case.id}: the library selects {code}, the table says {case.plan}"
    if case.stat_rows:
        assert rows == case.stat_rows
    assert before == {k: L.lib.vs_get_option(k.encode()) for k, _ in case.options}          # the options are put back
    if case.inst is not None and len(case.inst) == 6:       # a tile row: its shape is ragged in every direction the instantiation tiles
        bn, pt, nw, taps, stride, dil = case.inst
        tw = (8 if pt == 1 else 16) if stride == 1 else (16 if case.wout >= 16 else 8)
        th = nw * 16 * pt // tw
        assert (taps, stride, dil) == (case.k * case.k, case.stride, case.dilation)
        assert case.wout > tw and case.wout % tw and case.hout % th and case.cout > bn and case.cout % bn
        assert case.hout > th or (case.h, case.w) == (7, 9)          # (the 1x1 rows of the 64-pixel tiles: 7 rows of one 8-row tile)
        assert case.cin > CC.CHUNK[case.code] and case.cin % CC.CHUNK[case.code] and case.n in (2, 3)


@pytest.mark.parametrize("case", CC.CASES, ids=lambda c: c.id)
def test_reference_and_bound_on_the_cpu(case):
    ref, bound = CC.reference(case)
    failed = []
    # the reference against an independent float64 evaluation
    other = CC.independent_reference(case)
    rel = ((ref - other).abs().max() / ref.abs().max()).item()
    print(f"{case.id}: reference against unfold + einsum {rel:.3g} relative")
    if not rel <= 1e-12:
        failed.append(("reference", rel))
    # the bound can be met: fp32 on the CPU, rounded to the stored type
    honest = CC.figure(CC.cpu_fp32(case), case)
    print(f"{case.id}: fp32 CPU convolution {honest:.3g} of the bound")
    if not honest <= 1.0:
        failed.append(("honest", honest))
    # the bound has teeth
    for mutation in ("chunks", "channel", "tail"):
        fig = CC.figure(CC.cpu_fp32(case, mutation), case)
        # rounding the accumulator to the storage type is no mutation of an fp32 launch, and shows only where there are several chunks
        required = mutation != "chunks" or (case.cin >= 128 and case.code != 0)
        print(f"{case.id}: mutation {mutation} {fig:.3g} of the bound ({'required' if required else 'reported'})")
        if required and not fig > 1.0:
            failed.append((mutation, fig))
    # never looser than the tolerance it replaces (16-bit types; fp32 keeps the old tolerance as well)
    if case.code != 0:
        looser = (bound / CC.old_tolerance(case)).max().item()
        print(f"{case.id}: bound at most {looser:.3g} of the old tolerance")
        if not looser <= 1.0:
            failed.append(("looser", looser))
    assert bool((bound > 0).all()) and bool(torch.isfinite(bound).all())
    assert not failed, (case.id, failed)
