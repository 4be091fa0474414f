"""The cases, reference and bound of tests/wgrad_cases.py without a GPU: the table against a hand-written list of the instantiations
dispatch() of csrc/conv_wgrad.hip builds and against the library's own plan query (host logic), the shapes against the tile sizes
(every instantiation row is ragged in every direction its kernel tiles), the float64 reference against an independent float64
evaluation, and the bound against fp32 torch on the CPU - an honest fp32 weight gradient meets it on every case, three seeded
mutations of that computation exceed it, and it is nowhere looser than the rtol / atol 1e-3 it replaces."""
import pytest
import torch

import wgrad_cases as WC
from hip_helpers import lib, option

G, FA = WC.GENERIC, WC.FAST
# conv_wgrad_kernel<T, WO, NTAPS, STRIDE, PT, DIL> / conv_wgrad_bf16_kernel<MO, NTAPS, STRIDE, PT, DIL> as dispatch() instantiates them,
# (wo, taps, stride, pt, dilation), written out from csrc/conv_wgrad.hip
TILED = [
    (4, 9, 1, 2, 1), (2, 9, 1, 2, 1), (1, 9, 1, 2, 1), (4, 1, 1, 2, 1), (2, 1, 1, 2, 1), (1, 1, 1, 2, 1),      # 128-pixel tiles
    (4, 9, 1, 1, 1), (2, 9, 1, 1, 1), (1, 9, 1, 1, 1), (4, 1, 1, 1, 1), (2, 1, 1, 1, 1), (1, 1, 1, 1, 1),      # 64-pixel tiles
    (4, 9, 2, 1, 1), (2, 9, 2, 1, 1), (1, 9, 2, 1, 1), (4, 1, 2, 1, 1), (2, 1, 2, 1, 1), (1, 1, 2, 1, 1),      # stride 2
    (4, 9, 1, 2, 2), (4, 9, 1, 1, 2), (2, 9, 1, 2, 2), (2, 9, 1, 1, 2),                                        # dilation 2
    (4, 9, 1, 1, 4), (2, 9, 1, 1, 4),                                                                          # dilation 4
]
# (family, dtype) the tiled kernels are built for; the ring kernel <MO, TWS, IMGS> as (mo, imgs); the row kernels as (form, wq)
BUILT_FOR = [(G, 0), (G, 1), (FA, 1)]
RING = [("ring", 4, 1), ("ring", 2, 1), ("ring", 1, 1), ("ring", 4, 2)]
ROWS = [("rows", form, wq) for form in (1, 2, 3) for wq in (1, 2, 4)]

ALL = WC.CASES + WC.REFUSED


def test_table_has_one_row_per_instantiation_and_dtype():
    assert len(TILED) == 24 and len(set(TILED)) == 24
    rows = [(c.inst, c.code) for c in WC.CASES if c.inst is not None]
    want = [((fam,) + t, code) for fam, code in BUILT_FOR for t in TILED] + [(r, 1) for r in RING + ROWS]
    assert sorted(rows, key=repr) == sorted(want, key=repr)
    assert len({c.id for c in ALL}) == len(ALL)
    # the instantiation a row stands for is the one its hand-written plan names
    for c in WC.CASES:
        p = c.plan
        if c.inst is None:
            continue
        if c.inst[0] == "ring":
            assert (p.family, p.wo, p.imgs) == (WC.RING,) + c.inst[1:]
        elif c.inst[0] == "rows":
            assert (p.family, p.rows_form, p.wq) == (WC.ROWS,) + c.inst[1:]
        else:
            assert (p.family, p.wo, p.taps, p.stride, p.pt, p.dil) == c.inst
    # the slab-reduce kernels and the extract; the split structure on a generic, a fast and a ring row
    assert {c.reduce_group for c in WC.CASES} == {-1, 0, 1, 4, 16}
    assert {(c.cg, c.plan.extract, c.code, c.stride) for c in WC.CASES if c.cg} == {(cg, int(cg < 32), code, s) for cg in (4, 8, 16, 32) for code in (0, 1) for s in (1, 2)}
    for fam in (WC.GENERIC, WC.FAST, WC.RING):
        mine = [c for c in WC.CASES if c.plan.family == fam and not c.cg]
        assert any(c.plan.nsplit == 1 for c in mine) and any(c.plan.tiles_per_split == 2 and c.plan.nsplit > 1 for c in mine)
        assert any(c.plan.tiles_per_split >= 3 and len(WC.split_pixels(c)[-1]) < c.plan.tiles_per_split for c in mine)
        assert {c.reduce_group for c in mine} == {-1, 0, 1, 4, 16}
        if fam != WC.GENERIC:
            assert {c.plan.xmode for c in mine} == {0, 1, 2}
    forms = {fam: {f for c in WC.CASES if c.plan.family == fam for f in ("up0", "c1") if getattr(c, f)} for fam in (WC.GENERIC, WC.FAST, WC.RING)}
    assert all(v == {"up0", "c1"} for v in forms.values()), forms
    assert {c.classes for c in WC.CASES if c.classes} == {1, 2, 4, 7}


@pytest.mark.parametrize("case", WC.CASES, ids=lambda c: c.id)
def test_plan_of_the_table_is_what_the_library_selects(case):
    L = lib()
    before = {k: L.lib.vs_get_option(k.encode()) for k, _ in case.options}
    rc, plan = WC.queried(L, case)
    assert rc == 0, L.last_error()
    assert plan == case.plan, f"{case.id}: the library selects {plan}, the table says {case.plan}"
    assert before == {k: L.lib.vs_get_option(k.encode()) for k, _ in case.options}          # the options are put back
    with option(**dict(case.options)):       # the workspace query the callers size their buffer with answers the plan's figure
        asked = (L.lib.vs_head_wgrad_planes_workspace(case.code, case.n, case.classes, case.h, case.w) if case.classes else
                 L.lib.vs_conv2d_wgrad_workspace(WC.descriptor(L, case)))
    assert asked == case.plan.workspace_bytes
    assert len(WC.split_pixels(case)) == case.plan.nsplit


@pytest.mark.parametrize("case", [c for c in WC.CASES if c.inst is not None], ids=lambda c: c.id)
def test_instantiation_rows_are_ragged_in_every_direction_the_kernel_tiles(case):
    p = case.plan
    if p.family == WC.ROWS:
        steps, per_image = case.n * case.hout // (2 if p.rows_form == 2 else 1), case.hout // (2 if p.rows_form == 2 else 1)
        assert case.wout == 128 * p.wq and case.n == 3
        assert steps % p.tiles_per_split and per_image % p.tiles_per_split          # a ragged last range; ranges that cross image boundaries
        return
    if p.imgs == 2:
        assert (case.hout, case.wout) == (8, 8) and case.n % 2 == 0 and case.n // 2 >= 3 and case.cout > 64 and case.cout % 64
        return
    tw = (16 if p.pt == 2 else 8) if case.stride == 1 else (16 if case.wout >= 16 else 8)
    th = 64 * p.pt // tw
    assert (p.taps, p.stride, p.dil) == (case.k * case.k, case.stride, case.dilation) and case.n == 3
    assert case.wout > tw and case.wout % tw and case.hout % th and case.cout > 16 * p.wo and case.cout % (16 * p.wo)
    assert case.hout > th or (case.h, case.w) == (7, 9)          # (the 1x1 rows of the 64-pixel tiles: 7 rows of one 8-row tile)
    if p.family == WC.RING:
        assert case.c0 % 32 == 0 and case.c1 % 32 == 0 and case.c1 > 0            # whole chunks only: the ring kernel takes no others
    else:
        assert case.cin > WC.CHUNK[case.code] and case.cin % WC.CHUNK[case.code]
        assert (case.cout % 8 != 0) == (p.family == WC.GENERIC and case.code == 1)  # bf16 reaches the generic kernel through cout % 8 only


@pytest.mark.parametrize("case", WC.CASES, ids=lambda c: c.id)
def test_reference_and_bound_on_the_cpu(case):
    ref, bound = WC.reference(case)
    assert tuple(ref.shape) == case.dw_shape
    failed = []
    # the reference against an independent float64 evaluation
    other = WC.independent_reference(case)
    rel = ((ref - other).abs().max() / ref.abs().max()).item()
    print(f"{case.id}: reference against unfold + einsum {rel:.3g} relative")
    if not rel <= 1e-12:
        failed.append(("reference", rel))
    # the bound can be met: fp32 autograd on the CPU
    honest = WC.figure(WC.cpu_fp32(case), case)
    print(f"{case.id}: fp32 CPU weight gradient {honest:.3g} of the bound (m = {WC.chain_roundings(case.code, case.plan)})")
    if not honest <= 1.0:
        failed.append(("honest", honest))
    # the bound has teeth
    for mutation in ("tail", "tile", "slab"):
        if mutation == "slab" and case.plan.nsplit == 1:
            continue
        fig = WC.figure(WC.cpu_fp32(case, mutation), case)
        print(f"{case.id}: mutation {mutation} {fig:.3g} of the bound")
        if not fig > 1.0:
            failed.append((mutation, fig))
    # never looser than the tolerance it replaces
    looser = (bound / WC.old_tolerance(case)).max().item()
    print(f"{case.id}: bound at most {looser:.3g} of the old tolerance")
    if not looser <= 1.0:
        failed.append(("looser", looser))
    assert bool((bound > 0).all()) and bool(torch.isfinite(bound).all())
    assert not failed, (case.id, failed)


@pytest.mark.parametrize("case", WC.REFUSED, ids=lambda c: c.id)
def test_refused_rows_are_refused_by_the_query(case):
    """the query returns the status the launch would return for a sufficient workspace: the rows that only withhold workspace answer
    their plan"""
    L = lib()
    rc, plan = WC.queried(L, case)
    if case.ws_short:
        assert rc == 0 and plan == case.plan
        return
    assert rc != 0 and L.last_error()
