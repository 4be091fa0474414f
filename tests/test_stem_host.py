"""The cases, reference and bound of tests/stem_cases.py without a GPU: the table against a hand-written list of the forms the launches of
csrc/stem.hip can select, the launch facts of its three shapes (tiles, tiles per weight-gradient range, the shorter last range, the
slab-reduce group, the workgroups that walk a second tile) recomputed from the kernels' constants, the float64 reference against an
independent float64 evaluation, and the bound against fp32 torch on the CPU - an honest fp32 evaluation meets it on every row, four
seeded mutations exceed it on every row they apply to, and it is nowhere looser than the tolerances it stands beside.  The launches
that must be refused are refused here too: the argument checks fire before anything touches a device."""
import pytest
import torch

import stem_cases as SC
from hip_helpers import lib

# what vs_stem_fwd, vs_stem_fwd_bins and vs_stem_wgrad select, written out from csrc/stem.hip: (kernel form, dtype, stem_bf16)
SELECTED = [
    ("fwd", 0, None),                 # stem_fwd_kernel<float>
    ("fwd", 1, 0),                    # stem_fwd_kernel<bf16_t>
    ("fwd", 2, None),                 # stem_fwd_kernel<f16_t>
    ("fwd-mfma16", 1, 1),             # stem_fwd_bf16_kernel, bins = nullptr
    ("fwd-bins", 1, 1),               # stem_fwd_bf16_kernel with bins
    ("wgrad", 0, None),               # stem_wgrad_kernel<float>
    ("wgrad", 1, 0),                  # stem_wgrad_kernel<bf16_t>
    ("wgrad-mfma16", 1, 1),           # stem_wgrad_bf16_kernel
]
EPILOGUES = [(0, 0), (1, 1), (0, 1)]      # (affine, relu): none, affine + ReLU, ReLU alone
ALL = SC.CASES + SC.REFUSED


def test_table_names_exactly_the_forms_the_launches_select():
    rows = {(c.form, c.code, dict(c.options).get("stem_bf16")) for c in SC.CASES}
    assert rows == set(SELECTED) and len(SELECTED) == 8
    assert set(SC.FORMS) == {f for f, _, _ in SELECTED}
    assert len({c.id for c in ALL}) == len(ALL)
    for form, code, opt in SELECTED:
        mine = [c for c in SC.CASES if (c.form, c.code, dict(c.options).get("stem_bf16")) == (form, code, opt)]
        epilogues = EPILOGUES if form in ("fwd", "fwd-mfma16") else EPILOGUES[:1]
        assert len(mine) == len(SC.SHAPES) * len(epilogues)
        assert {(c.shape, c.affine, c.relu) for c in mine} == {(s, a, r) for s in SC.SHAPES for a, r in epilogues}
    assert len(SC.CASES) == (3 + 1) * 9 + (1 + 2 + 1) * 3
    refused = {(c.label, c.form) for c in SC.REFUSED}
    assert {("refused-fp16-wgrad", "wgrad"), ("refused-odd-h-fwd", "fwd"), ("refused-odd-w-fwd", "fwd"), ("refused-workspace-a-byte-short", "wgrad"),
            ("refused-bins-fp32", "fwd-bins"), ("refused-bins-nb-12", "fwd-bins")} <= refused


@pytest.mark.parametrize("shape", SC.SHAPES, ids=lambda s: f"{s.n}x{s.h}x{s.w}")
def test_launch_facts_of_the_three_shapes(shape):
    """the hand-written structure of the table against the kernels' constants (8 x 32 tiles, grid min(tiles, 1024), kStemBlocks = 1024,
    the bf16 weight gradient's 512) and against slab_reduce_groups' rule"""
    tiles = SC.tile_count(shape.n, shape.h, shape.w)
    r32, r16 = SC.range_structure(tiles, SC.WGRAD_BLOCKS["wgrad"]), SC.range_structure(tiles, SC.WGRAD_BLOCKS["wgrad-mfma16"])
    print(f"{shape.n}x{shape.h}x{shape.w}: {tiles} tiles, walk {SC.cdiv(tiles, SC.FWD_BLOCKS)}, fp32 ranges {r32} group {SC.slab_group(r32[1])}, "
          f"bf16 ranges {r16} group {SC.slab_group(r16[1])}")
    assert tiles == shape.tiles
    assert shape.walk == SC.cdiv(tiles, SC.FWD_BLOCKS)
    assert r32 == shape.ranges32 and r16 == shape.ranges16
    assert (SC.slab_group(r32[1]), SC.slab_group(r16[1])) == (shape.group32, shape.group16)
    assert max(r32[1], r16[1]) * SC.DW * 4 <= lib().lib.vs_stem_wgrad_workspace(shape.n, shape.h, shape.w)


def test_the_shapes_cover_what_they_are_chosen_for():
    a, b, c = SC.SHAPES
    # ragged in both directions, more than one tile each way, a last column tile narrower than 16
    assert (a.h // 2) % SC.TPH and (a.w // 2) % SC.TPW and a.h // 2 > SC.TPH and a.w // 2 > SC.TPW and (a.w // 2) % SC.TPW < 16
    assert (b.h, b.w) == (2, 2) and b.tiles == b.n
    # a second tile for some workgroups of the forward walk but not for all; two and three tiles a range with a shorter last range
    assert SC.FWD_BLOCKS < c.tiles < 2 * SC.FWD_BLOCKS and c.tiles - SC.FWD_BLOCKS == 7
    assert c.ranges32 == (2, 516, 1) and c.ranges16 == (3, 344, 2)
    assert {a.group32, b.group32, c.group32} == {1, 4, 16} == {a.group16, b.group16, c.group16}
    assert c.n * (c.h // 2) * (c.w // 2) * 64 == 395904 and c.n * c.h * c.w == 24744
    for s in SC.SHAPES:
        case = next(k for k in SC.CASES if k.shape == s)
        assert len(SC.tiles_of(case)) == s.tiles


@pytest.mark.parametrize("case", SC.CASES, ids=lambda c: c.id)
def test_reference_and_bound_on_the_cpu(case):
    ref, bound = SC.reference(case)
    failed = []
    other = SC.independent_reference(case)
    rel = ((ref - other).abs().max() / ref.abs().max()).item()
    print(f"{case.id}: reference against unfold + einsum {rel:.3g} relative")
    if not rel <= 1e-12:
        failed.append(("reference", rel))
    honest = SC.figure(SC.cpu_fp32(case), case)
    print(f"{case.id}: fp32 CPU evaluation {honest:.3g} of the bound")
    if not honest <= 1.0:
        failed.append(("honest", honest))
    for mutation in SC.MUTATIONS:
        if not SC.applies(mutation, case):
            continue
        fig = SC.figure(SC.cpu_fp32(case, mutation), case)
        print(f"{case.id}: mutation {mutation} {fig:.3g} of the bound")
        if fig <= 1.0:              # (an unwritten tile is NaN, which no bound admits)
            failed.append((mutation, fig))
    if case.form != "fwd-bins":
        looser = (bound / SC.old_tolerance(case)).max().item()
        print(f"{case.id}: bound at most {looser:.3g} of the tolerance beside it")
        if not looser <= 1.0:
            failed.append(("looser", looser))
    assert bool((bound > 0).all()) and bool(torch.isfinite(bound).all())
    assert not failed, (case.id, failed)


@pytest.mark.parametrize("case", SC.REFUSED, ids=lambda c: c.id)
def test_refused_rows_are_refused_before_any_launch(case):
    """VS_REQUIRE / VS_NO_F16 / stem_fwd_bins_ok return before the first HIP call, so the status is the same on a host without a GPU; the
    buffers are host memory of the right size and stay as they were"""
    L = lib()
    s = case.shape
    x, w = torch.zeros(s.n, 1, s.h, s.w), torch.zeros(64, 49)
    out = torch.full((SC.out_elems(case),), -77.0)
    dy = torch.zeros(s.n, s.h // 2, s.w // 2, 64) if case.is_wgrad else None
    asked = L.lib.vs_stem_wgrad_workspace(s.n, s.h, s.w)
    ws = torch.full((asked // 4,), -77.0) if case.is_wgrad else None
    bins = torch.zeros(16, 2, 64, dtype=torch.int64) if case.form == "fwd-bins" else None
    before = {k: L.lib.vs_get_option(k.encode()) for k, _ in case.options}
    rc = SC.launch(L, case, x, w, out, dy=dy, ws=ws, ws_bytes=asked - case.ws_short, bins=bins)
    assert rc != 0 and L.last_error()
    assert rc == (-3 if case.label.startswith("refused-bins-") and case.nb == SC.NB else -1), (rc, L.last_error())
    assert before == {k: L.lib.vs_get_option(k.encode()) for k, _ in case.options}
    assert bool((out == -77.0).all()) and (ws is None or bool((ws == -77.0).all())) and (bins is None or not bins.any())
