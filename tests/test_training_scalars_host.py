"""The references of tests/training_scalar_cases.py, checked without a GPU: the float64 loss restatements against the reference
project's own numbers (g10), the NumPy AdamW against torch.optim.AdamW, and the cases themselves - each must be one on which plain
float32 arithmetic already sits well inside the bounds the kernels are held to, so that a kernel outside them is wrong and not unlucky."""
import numpy as np
import pytest
import torch

import training_scalar_cases as T


# ---- anchors ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("classes", [1, 2, 4])
def test_float64_restatements_reproduce_the_reference_project(golden, classes):
    """every criterion and class count of g10_losses.npz (BCEDiceLoss(0.75, 0.25), BCE, generalised Dice, cross entropy; gradient of
    1.3 x loss), within the bounds tests/test_hip_ops.py holds the kernels to on the same file"""
    g = golden("g10_losses.npz")
    logits, targets = g[f"k{classes}__logits"], g[f"k{classes}__targets"]
    names = [n for n in T.CRITERIA if f"k{classes}__{n}__loss" in g.files]
    assert names == [n for n in T.CRITERIA[1:] if not (n == "CrossEntropyLoss" and classes == 1)]
    for name in names:
        loss, grad = T.evaluate(name, logits, targets, torch.float64)
        ref_l, ref_g = float(g[f"k{classes}__{name}__loss"]), g[f"k{classes}__{name}__grad"].astype(np.float64)
        assert abs(loss - ref_l) <= 2e-6 * max(1.0, abs(ref_l)), (name, loss, ref_l)
        err = np.abs(1.3 * grad - ref_g).max()
        assert err <= 2e-5 * np.abs(ref_g).max(), (name, err, np.abs(ref_g).max())


def test_default_dice_restatement_is_the_normalization_none_of_the_selectable_dice():
    """oracle.predictor_numpy.dice_loss_none (pinned to the reference project by golden g6) and data/losses.py's DiceLoss agree in
    float64: BCEDiceLoss's Dice term, anchored above, is the same code behind a sigmoid"""
    from volume_segmantics_amd.data.losses import DiceLoss
    logits, targets = T.inputs(T.Case("small_odd", 3))
    x, t = torch.tensor(logits).double(), torch.tensor(targets)
    assert float(T.criterion_fn("Dice")(x, t)) == pytest.approx(float(DiceLoss(normalization="none")(x, t)), abs=1e-14)


def test_numpy_adamw_is_torch_adamw_in_float64():
    """five steps on a float64 parameter, lr and beta1 changing each step as OneCycleLR moves them: p, exp_avg, exp_avg_sq within 1e-12
    relative (elementwise for p and exp_avg_sq; exp_avg, a difference of two terms in torch's lerp form, relative to its largest)"""
    rng = np.random.default_rng(5)
    n = 1000
    p0 = rng.standard_normal(n)
    p_t = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
    b2, eps, wd = T.f32(0.999), T.f32(1e-8), T.f32(0.01)
    opt = torch.optim.AdamW([p_t], lr=1e-3, betas=(0.9, b2), eps=eps, weight_decay=wd, foreach=False)
    p, m, v = p0.copy(), np.zeros(n), np.zeros(n)
    for step in range(1, 6):
        lr, b1 = T.f32(1e-3 * step * (6 - step)), T.f32(0.95 - 0.025 * step)
        g = rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 2, n)
        g[::17] = 0.0
        opt.param_groups[0]["lr"], opt.param_groups[0]["betas"] = lr, (b1, b2)
        p_t.grad = torch.tensor(g)
        opt.step()
        p, m, v = T.adamw_reference(p, g, m, v, lr, b1, b2, eps, wd, step)
        state = opt.state[p_t]
        assert float(state["step"]) == step
        assert (np.abs(p - p_t.detach().numpy()) <= 1e-12 * np.abs(p)).all()
        m_t, v_t = state["exp_avg"].numpy(), state["exp_avg_sq"].numpy()
        assert np.abs(m - m_t).max() <= 1e-12 * np.abs(m_t).max()
        assert (np.abs(v - v_t) <= 1e-12 * np.abs(v_t)).all()


def test_adamw_reference_leaves_masked_elements_alone():
    p, g, m, v = (np.arange(1, 5, dtype=np.float64) * s for s in (1.0, 0.5, 0.1, 0.01))
    mask = np.array([1, 0, 1, 0], dtype=np.uint8)
    p1, m1, v1 = T.adamw_reference(p, g, m, v, 1e-3, 0.9, 0.999, 1e-8, 0.01, 3, mask)
    full = T.adamw_reference(p, g, m, v, 1e-3, 0.9, 0.999, 1e-8, 0.01, 3)
    for got, all_, old in zip((p1, m1, v1), full, (p, m, v)):
        assert np.array_equal(got[[1, 3]], old[[1, 3]]) and np.array_equal(got[[0, 2]], all_[[0, 2]]) and not np.array_equal(all_, old)


# ---- the cases -------------------------------------------------------------------------------------------------------------------
def test_case_inputs_are_what_the_cases_say():
    for case in T.LOSS_CASES:
        logits, targets = T.inputs(case)
        n, h, w = case.nhw
        assert logits.shape == targets.shape == (n, case.classes, h, w) and logits.dtype == np.float32
        assert targets.dtype == (np.uint8 if case.tdtype == "uint8" else np.float32) and set(np.unique(targets)) <= {0, 1}
        per_class = targets.reshape(n, case.classes, -1).sum(-1)
        for c in range(case.classes):
            assert (per_class[:, c] == 0).all() == (c == case.absent_class), (case.id, c)
        column = targets.sum(1)
        if case.zero_column:
            assert (column.reshape(n, -1)[:, ::7] == 0).all() and (column == 1).sum() > column.size // 2
        elif case.classes > 1:
            assert (column == 1).all()
        if case.dead == "zero":
            assert (logits[:, case.absent_class] == 0).all()
        if case.dead in ("off", "faint"):
            assert (logits[:, case.absent_class] == (-120 if case.dead == "off" else -40)).all()
        if case.saturate:
            assert set(np.unique(np.abs(logits[:, :, :6]))) == {90.0} and (logits[:, :, :6] > 0).any() and (logits[:, :, :6] < 0).any()
    ids = [T.loss_id(p) for p in T.LOSS_PARAMS]
    assert len(set(ids)) == len(ids)
    # the matrix the cases must span
    on_small = [c for c in T.LOSS_CASES if c.shape == "small_odd"]
    assert {c.classes for c in on_small} == {1, 2, 3, 5, 16}
    assert {c.classes for c in T.LOSS_CASES if c.shape == "stride_vec"} == {2, 5}
    assert {c.absent for c in on_small} == {None, 0, "last"} and {c.scale for c in on_small} == {1.0, 30.0}
    assert any(c.saturate for c in on_small) and any(c.zero_column for c in on_small)
    for shape in ("small_odd", "one_wave", "stride_odd", "stride_vec"):
        assert {c.tdtype for c in T.LOSS_CASES if c.shape == shape} == {"uint8", "float32"}
    assert all(c.shape == "small_odd" for c in T.LOSS_CASES if c.absent is not None or c.scale != 1 or c.saturate or c.zero_column)


@pytest.mark.parametrize("param", [p for p in T.LOSS_PARAMS if p[0].tdtype == "uint8" or p[0].base not in T.LOSS_CASES], ids=T.loss_id)
def test_float32_restatement_sits_within_a_quarter_of_the_bounds(param):
    """The condition on a case: the same torch restatement evaluated in float32 on the CPU lies within a quarter of the bounds the
    kernels get, measured against float64.  A case that fails this is replaced by other inputs; the bound stays."""
    case, name = param
    logits, targets = T.inputs(case)
    ref_loss, ref_grad = T.reference(case, name)
    loss, grad = T.evaluate(name, logits, targets, torch.float32)
    for label, err, bound in T.loss_errors(loss, grad, ref_loss, ref_grad):
        print(f"{case.id} {name} float32 {label}: {err:.3e} of {bound:.3e}")
        assert err <= 0.25 * bound, (label, err, bound)


def test_exactly_one_family_has_an_identically_zero_gradient():
    """Dice 'none' on one class with no foreground: I = 0 and t = 0 everywhere, so d loss / d logits is zero in exact arithmetic and
    the relative gradient bound of the GPU test is 0 there - the kernel must return zeros.  No other (case, criterion) is like that."""
    zero = set()
    for case, name in T.LOSS_PARAMS:
        if case.tdtype == "uint8" or case.base not in T.LOSS_CASES:
            if not T.reference(case, name)[1].any():
                zero.add((case.classes, case.absent_class, name))
    assert zero == {(1, 0, "Dice")}
    assert sum(1 for c in T.LOSS_CASES if c.classes == 1 and c.absent_class == 0) >= 2


def test_iou_logits_have_exact_ties_and_no_near_ties():
    for shape in T.IOU_SHAPES:
        for classes in T.IOU_CLASSES:
            x, probs, onehot, ref = T.iou_inputs(shape, classes)
            assert torch.equal(x * 8, torch.round(x * 8)) and 0.0 <= ref <= 1.0
            if classes > 1:
                top2 = torch.topk(x, 2, dim=1).values
                tied = top2[:, 0] == top2[:, 1]
                assert tied.any() and (top2[:, 0] - top2[:, 1])[~tied].min() >= 0.125
                # the probabilities decide as the logits do: the first maximum
                assert torch.equal(torch.argmax(probs, 1), torch.argmax(x, 1))
                ptop = torch.topk(probs, 2, dim=1).values
                assert torch.equal(ptop[:, 0] == ptop[:, 1], tied)


def test_onehot_reference_zeroes_columns_of_labels_past_the_classes():
    for classes in T.ONEHOT_CLASSES:
        labels = T.onehot_labels("small_odd", classes)
        ref = T.onehot_reference(labels, classes, rows=5).numpy()
        assert ref.shape == (3, classes, 33, 31) and ref.dtype == np.uint8
        assert np.array_equal(ref.sum(1), (labels < classes).astype(np.uint8)) and (labels >= classes).any() and (labels < classes).any()
        assert np.array_equal(np.where(labels < classes, ref.argmax(1), labels), labels)


def test_adamw_inputs_span_what_the_kernel_must_take():
    n = T.ADAMW_SIZES[1]
    p0, mask, grads = T.adamw_inputs(n)
    assert n > 8192 * 256 and T.ADAMW_SIZES[0] == 1 and 0 < mask.sum() < n
    mags = np.abs(np.concatenate(grads))
    assert (mags == 0).any() and mags[mags > 0].min() <= 1.01e-12 and mags.max() >= 0.99e3 and mags.max() <= 1e3
    signs = np.stack([np.sign(g) for g in grads])
    assert not ((signs > 0).any(0) & (signs < 0).any(0)).any()           # no element changes the sign of its gradient
    steps = [s[0] for s in T.ADAMW_SCHEDULE]
    assert steps == [1, 2, 3, 4, 5, 6, 1000, 100000] and any(s[3] for s in T.ADAMW_SCHEDULE)
    assert len({s[1] for s in T.ADAMW_SCHEDULE[:6]}) == 6 and len({s[2] for s in T.ADAMW_SCHEDULE[:6]}) > 3


def test_float32_adamw_sits_inside_its_bounds():
    """the kernel's expression tree in NumPy float32 (no fused multiply-adds) with the host's float32 bias corrections: inside the
    moment and update bounds on the small run, so the bounds are ones float32 arithmetic can meet"""
    n = 10007
    p0, mask, grads = T.adamw_inputs(n)
    F = np.float32
    p, m, v = p0.copy(), np.zeros(n, F), np.zeros(n, F)
    b2, eps, wd = F(T.ADAMW_BETA2), F(T.ADAMW_EPS), F(T.ADAMW_WD)
    for (step, lr, b1, masked), g in zip(T.ADAMW_SCHEDULE, grads):
        lr, b1 = F(lr), F(b1)
        h = T.host_hyper(lr, b1, b2, eps, wd, step)
        before = (p.copy(), m.copy(), v.copy())
        keep = (mask != 0) if masked else np.ones(n, bool)
        pn = p * (F(1) - lr * wd)
        mn = b1 * m + (F(1) - b1) * g
        vn = b2 * v + (F(1) - b2) * g * g
        pn = pn - (lr / h[5]) * (mn / (np.sqrt(vn) / h[6] + eps))
        assert pn.dtype == mn.dtype == vn.dtype == np.float32
        p, m, v = np.where(keep, pn, p), np.where(keep, mn, m), np.where(keep, vn, v)
        figures, changed = T.adamw_step_figures(before, (p, m, v), g, tuple(float(x) for x in (lr, b1, b2, eps, wd)), step,
                                                mask if masked else None)
        assert changed == 0
        for label, ratio in figures:
            print(f"step {step} {label}: {ratio:.3f} of the bound")
            assert ratio <= 1.0, (step, label, ratio)


def test_host_hyper_is_float32_arithmetic():
    for lr, b1, b2, eps, wd, step in T.HYPER_CASES:
        h = T.host_hyper(T.f32(lr), T.f32(b1), T.f32(b2), T.f32(eps), T.f32(wd), step)
        assert h.dtype == np.float32 and h[7] == step and h[0] == np.float32(lr) and h[1] == np.float32(b1)
        exact1 = 1.0 - float(np.float32(b1)) ** step
        exact2 = np.sqrt(1.0 - float(np.float32(b2)) ** step)
        assert abs(h[5] - exact1) <= 4e-6 * exact1 and abs(h[6] - exact2) <= 4e-6 * exact2
