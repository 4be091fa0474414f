"""-m gpu: training on partly labelled volumes on the MI355X - the _masked entry points of csrc/loss.hip (default Dice, BCE-Dice, BCE,
cross entropy, generalised Dice, MeanIoU) and vs_onehot_valid_u8 against the compaction oracle of tests/sparse_label_cases.py, at the
smallest shapes that reach each launch path; bit-equality with the unmasked entry points under an all-ones mask; the device
augmentation on masks that hold 255; one trainer-level run from a sparsely labelled volume.

    small_odd (3, 33, 31)       scalar kernels, ragged last workgroup; classes 1, 2, 3, 5, 16; every mask pattern
    one_wave (1, 5, 7)          a single wave
    misaligned (2, 32, 32)      hw % 4 == 0, everything aligned: the uchar4 loads of the mask, valid and ignored pixels mixed inside
                                one vector; the mask pointer one byte in: must take the scalar kernels and still be right
    stride_vec (5, 660, 640)    K = 2 and 5: second grid-stride trips of the vector reductions and gradients, mask loads crossing
                                sample boundaries (every 8th row valid, and 30 % at random)"""
import logging

import numpy as np
import pytest
import torch

import sparse_label_cases as S
import training_scalar_cases as T

pytestmark = pytest.mark.gpu


def _held(figures, context):
    failed = []
    for label, err, bound in figures:
        print(f"{context} {label}: {err:.3e} of {bound:.3e}")
        if not err <= bound:
            failed.append((label, err, bound))
    assert not failed, (context, failed)


PATTERN_CASES = [(T.Case("small_odd", k, tdtype=td), p) for k in (1, 2, 3, 5, 16) for p in S.PATTERNS
                 for td in (("uint8", "float32") if k in (1, 3) else ("uint8",))]
PATH_CASES = [(T.Case("one_wave", 1), "random30"), (T.Case("one_wave", 3, tdtype="float32"), "random30"),
              (T.Case("misaligned", 3), "random30"), (T.Case("misaligned", 3, tdtype="float32"), "random30"),
              (T.Case("small_odd", 1), "foreground_only"), (T.Case("misaligned", 1, tdtype="float32"), "foreground_only"),
              (T.Case("misaligned", 3), "sample_out"), (T.Case("misaligned", 1), "class_absent"), (T.Case("misaligned", 3), "none"),
              (T.Case("stride_vec", 2), "rows8"), (T.Case("stride_vec", 2, tdtype="float32"), "rows8"),
              (T.Case("stride_vec", 5), "rows8"), (T.Case("stride_vec", 5, tdtype="float32"), "rows8"),
              (T.Case("stride_vec", 2), "random30"), (T.Case("stride_vec", 5), "random30")]
MASKED_PARAMS = [(case, pattern, name) for case, pattern in PATTERN_CASES + PATH_CASES for name in T.criteria_of(case)]
MASKED_PARAMS.sort(key=lambda p: (p[0].shape, p[0].classes, p[1], T.CRITERIA.index(p[2]), p[0].tdtype))   # one reference, then its uses


def _masked_id(param):
    return f"{param[0].id}-{param[1]}-{param[2]}"


@pytest.mark.parametrize("param", MASKED_PARAMS, ids=_masked_id)
def test_masked_loss_and_gradient_against_the_compaction_oracle(param):
    """HipDiceLoss / HipSegLoss with `valid` (autograd, 1.7 x loss) and the C ABI with a null grad_out into a NaN-filled dlogits:
    the bounds of training_scalar_cases against the float64 reference on the valid pixels alone; every ignored element of the
    gradient is the bit pattern of +0.0; nothing is non-finite - with no valid pixel either, where the loss is the defined one.

    One-channel generalised Dice: where every valid pixel is foreground (one_pixel, foreground_only) the foreground gradient is the
    difference of terms a million times its size; the masked form keeps the foreground coefficient apart (csrc/loss.hip,
    seg_finalize_kernel) and these cases hold it to the same relative bound, whose scale is then that small gradient alone."""
    case, pattern, name = param
    _held(S.masked_figures(case, pattern, name), _masked_id(param))


@pytest.mark.parametrize("name", T.CRITERIA)
@pytest.mark.parametrize("tdtype", ["uint8", "float32"])
def test_mask_pointer_off_4_bytes_takes_the_scalar_kernels(tdtype, name):
    case = T.Case("misaligned", 3, tdtype=tdtype)
    _held(S.masked_figures(case, "random30", name, valid_offset=1), f"mask+1byte {tdtype} {name}")


@pytest.mark.parametrize("param", T.LOSS_PARAMS, ids=T.loss_id)
def test_all_ones_mask_returns_the_unmasked_bits(param):
    """loss and every gradient element, over every case the unmasked kernels are pinned on: the masked instantiations sum the same
    terms in the same order"""
    case, name = param
    logits, targets = T.inputs(case)
    ones = np.ones(case.nhw, np.uint8)
    for grad_out in (None, T.GRAD_OUT):
        loss, grad = T.abi_loss(name, logits, targets, grad_out)
        mloss, mgrad = S.abi_loss_masked(name, logits, targets, ones, grad_out)
        assert np.float32(loss).view(np.uint32) == np.float32(mloss).view(np.uint32), (loss, mloss)
        assert np.array_equal(grad.view(np.uint32), mgrad.view(np.uint32))


@pytest.mark.parametrize("classes", (2, 7, 254))
@pytest.mark.parametrize("shape", ("small_odd", "misaligned", "stride_vec"))
def test_onehot_valid_writes_the_onehot_bytes_and_the_mask(shape, classes):
    """hw % 4 != 0 (scalar branch) and == 0 (uchar4 branch, second trip at 660 x 640)"""
    from volume_segmantics_amd import _lib as L
    labels = T.onehot_labels(shape, classes).copy()
    labels[np.random.default_rng(classes).random(labels.shape) < 0.4] = S.IGNORE
    lab = torch.tensor(labels).to(T.DEV)
    n, hw = lab.shape[0], lab[0].numel()
    onehot = torch.full((n, classes) + tuple(lab.shape[1:]), 0xAB, dtype=torch.uint8, device=T.DEV)
    valid = torch.full_like(lab, 0xAB)
    L.check(L.lib.vs_onehot_valid_u8(L.ptr(lab), n, classes, hw, S.IGNORE, L.ptr(onehot), L.ptr(valid), None))
    torch.cuda.synchronize()
    assert torch.equal(onehot, T.onehot_device(labels, classes))
    assert np.array_equal(valid.cpu().numpy(), (labels != S.IGNORE).astype(np.uint8))
    assert not onehot.cpu().numpy()[np.broadcast_to(labels[:, None] == S.IGNORE, onehot.shape)].any()


def test_prepare_training_batch_with_an_ignore_label_on_the_device():
    from volume_segmantics_amd.utilities.base_data_utils import prepare_training_batch
    labels = np.random.default_rng(5).integers(0, 3, (3, 32, 32)).astype(np.uint8)
    labels[:, ::3] = S.IGNORE
    batch = (torch.zeros((3, 1, 32, 32), device=T.DEV), torch.tensor(labels).to(T.DEV))
    inputs, targets, valid = prepare_training_batch(batch, T.DEV, 3, ignore_label=S.IGNORE)
    assert targets.is_cuda and valid.is_cuda and valid.dtype == torch.uint8 and valid.shape == (3, 32, 32)
    cpu = prepare_training_batch((batch[0].cpu(), batch[1].cpu()), "cpu", 3, ignore_label=S.IGNORE)
    assert torch.equal(targets.cpu(), cpu[1]) and torch.equal(valid.cpu(), cpu[2])
    assert len(prepare_training_batch(batch, T.DEV, 3)) == 2


@pytest.mark.parametrize("tdtype", ["uint8", "float32"])
@pytest.mark.parametrize("classes", (1, 2, 3, 16))
@pytest.mark.parametrize("shape", T.IOU_SHAPES)
def test_masked_mean_iou_against_the_oracle(shape, classes, tdtype):
    """probabilities and logits; a whole sample ignored is left out of the mean; no valid pixel at all is NaN"""
    from volume_segmantics_amd.data.losses import MeanIoU
    x, probs, onehot, _ref = T.iou_inputs(shape, classes)
    case = T.Case(shape, classes)
    t = (onehot if tdtype == "uint8" else onehot.float()).to(T.DEV)
    for pattern in ("random30", "rows8", "sample_out", "one_pixel", "none"):
        valid = S.valid_mask(case, pattern)
        v = torch.tensor(valid).to(T.DEV)
        ref = S.iou_reference(probs, onehot, valid)
        ref_logits = ref if classes > 1 else S.iou_reference(torch.ones(onehot.shape), onehot, valid)
        got, got_logits = MeanIoU()(probs.to(T.DEV), t, v).item(), MeanIoU().from_logits(x.to(T.DEV), t, v).item()
        if not valid.any():
            assert np.isnan(ref) and np.isnan(got) and np.isnan(got_logits)
            continue
        _held([("probabilities", abs(got - ref), T.IOU_BOUND), ("from_logits", abs(got_logits - ref_logits), T.IOU_BOUND)],
              f"masked mean_iou {shape} k{classes} {tdtype} {pattern}")
    ones = torch.ones(case.nhw, dtype=torch.uint8, device=T.DEV)
    assert MeanIoU()(probs.to(T.DEV), t, ones).item() == MeanIoU()(probs.to(T.DEV), t).item()


def test_device_augmentation_keeps_mask_values():
    """csrc/augment.hip resamples masks nearest-neighbour with reflect-101 borders: {0, 1, 255} in, {0, 1, 255} out, for every branch
    that moves mask pixels, and over random draws of the whole pipeline"""
    from volume_segmantics_amd.data.gpu_augment import augment_batch
    size = 64
    sets = S.augment_param_sets(size)
    pairs = [S.sparse_mask_image(size, seed) for seed in range(len(sets))]
    images = torch.tensor(np.stack([p[0] for p in pairs])).to(T.DEV)
    masks = torch.tensor(np.stack([p[1] for p in pairs])).to(T.DEV)
    _x, out = augment_batch(images, masks, None, params=list(sets.values()))
    out = out.cpu().numpy()
    assert out.shape == (len(sets), size, size) and set(np.unique(out)) <= {0, 1, S.IGNORE}
    for j, branch in enumerate(sets):
        assert (out[j] == S.IGNORE).any() and (out[j] != S.IGNORE).any(), branch
    rng = np.random.default_rng(21)
    for _ in range(4):
        assert set(np.unique(augment_batch(images, masks, rng)[1].cpu().numpy())) <= {0, 1, S.IGNORE}


def _sparse_cube(cube=64, seed=3):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((cube,) * 3).astype(np.float32)
    for _ in range(3):
        for ax in range(3):
            v = (np.roll(v, 1, ax) + 2 * v + np.roll(v, -1, ax)) / 4
    dense = (v > np.percentile(v, 65)).astype(np.uint8)
    labels = np.full_like(dense, 7)                                   # 7 = "not labelled" in the input volume
    labels[::8] = dense[::8]
    noisy = v / np.abs(v).max() * 90 + 128 + rng.standard_normal(v.shape) * 8
    return np.clip(noisy, 0, 255).astype(np.uint8), labels


@pytest.mark.parametrize("step_mode", ["eager", "graph"])
def test_trainer_from_a_sparsely_labelled_volume(tmp_path, caplog, step_mode):
    """every 8th z-slice of a 64^3 volume labelled: one frozen epoch after a one-epoch LR finder, U-Net / resnet18; the samples are
    the slices with a label, the losses are finite, the checkpoint has K = 2 classes; `step_mode: graph` falls back to the
    call-by-call step and says so once"""
    from pathlib import Path
    from volume_segmantics_amd.data import TrainingDataSlicer, get_settings_data, volume_feed
    from volume_segmantics_amd.model.model_2d import create_model_from_file
    from volume_segmantics_amd.model.operations.vol_seg_2d_trainer import VolSeg2dTrainer
    s = get_settings_data(Path(__file__).resolve().parent.parent / "volseg-settings" / "2d_model_train_settings.yaml")
    s.image_size, s.precision, s.batch_size, s.lr_find_epochs, s.ignore_label, s.step_mode = 64, "fp32", 8, 1, 7, step_mode
    s.model = dict(s.model, encoder_name="resnet18", encoder_weights=None)
    data, labels = _sparse_cube()
    kept = S.kept_slices(labels, 7)
    assert [len(kept[a]) for a in "zyx"] == [8, 64, 64]
    slicer = TrainingDataSlicer(data, labels, s)
    assert slicer.num_seg_classes == 2 and set(np.unique(slicer.seg_vol)) == {0, 1, S.IGNORE}
    torch.manual_seed(11)
    trainer = VolSeg2dTrainer.from_volumes([slicer], slicer.num_seg_classes, s)
    assert isinstance(trainer.training_loader, volume_feed.VolumeSliceLoader) and trainer.ignore_label == S.IGNORE
    assert len(trainer.training_loader.table) + len(trainer.validation_loader.table) == 136
    assert trainer.training_loader.max_label == 1
    out = tmp_path / "sparse_model.pytorch"
    with caplog.at_level(logging.INFO):
        trainer.train_model(out, 1, s.patience, create=True, frozen=True)
    print(f"[sparse labels] {step_mode}: train {trainer.avg_train_losses}, valid {trainer.avg_valid_losses}, score {trainer.avg_eval_scores}")
    assert len(trainer.avg_train_losses) == 1
    assert np.isfinite(trainer.avg_train_losses[0]) and np.isfinite(trainer.avg_valid_losses[0]) and np.isfinite(trainer.avg_eval_scores[0])
    assert sum("call by call" in r.getMessage() for r in caplog.records) == (1 if step_mode == "graph" else 0)
    _model, num_labels, _codes = create_model_from_file(out)
    assert num_labels == 2
