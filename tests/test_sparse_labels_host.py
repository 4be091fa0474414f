"""Training on partly labelled volumes (settings key `ignore_label`), the parts that need no GPU: the torch restatements of the masked
criteria against the compaction oracle of tests/sparse_label_cases.py, the rule for a batch without a labelled pixel, the slicer's
relabelling and refusals, the slices left out of a run on both routes, the label-range checks, the host augmentation, and the
untouched behaviour without the key."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from torch import nn

import sparse_label_cases as S
import training_scalar_cases as T
import volume_feed_cases as V

HOST_CASES = (T.Case("small_odd", 1), T.Case("small_odd", 2), T.Case("small_odd", 3), T.Case("small_odd", 5), T.Case("one_wave", 3))
# both sides are float64 sums of the same terms in different orders: n k h w <= 15345 terms of magnitude O(1), 1e-16 each
F64_BOUND = 1e-11


def _settings(ignore=None, axes="All", **extra):
    return V.settings(axes, **({} if ignore is None else {"ignore_label": ignore}), **extra)


@pytest.mark.parametrize("pattern", [p for p in S.PATTERNS if p != "none"])
@pytest.mark.parametrize("case", HOST_CASES, ids=lambda c: c.id)
def test_restatements_with_a_mask_equal_the_reference_on_the_valid_pixels(case, pattern):
    logits, onehot, valid = S.masked_inputs(case, pattern)
    for name in T.criteria_of(case):
        ref_loss, ref_grad = S.reference(case, pattern, name)
        loss, grad = S.restatement_evaluate(name, logits, onehot, valid)
        assert abs(loss - ref_loss) <= F64_BOUND * max(1.0, abs(ref_loss)), (name, loss, ref_loss)
        assert np.abs(grad - ref_grad).max() <= F64_BOUND * max(np.abs(ref_grad).max(), 1e-300), name
        assert not grad[np.broadcast_to(valid[:, None] == 0, grad.shape)].any(), name


@pytest.mark.parametrize("case", HOST_CASES[:3], ids=lambda c: c.id)
def test_no_valid_pixel_gives_the_defined_losses_and_zero_gradients(case):
    """BCE and cross-entropy terms 0, Dice terms 1 (every denominator clamped), all gradients 0, nothing NaN - also with non-finite
    logits, which an ignored pixel must keep out of every sum"""
    logits, onehot, valid = S.masked_inputs(case, "none")
    poisoned = logits.copy()
    poisoned[0, 0, 0, :3] = (np.nan, np.inf, -np.inf)
    for name in T.criteria_of(case):
        for x in (logits, poisoned):
            loss, grad = S.restatement_evaluate(name, x, onehot, valid, torch.float32)
            assert loss == pytest.approx(S.M0_LOSS[name], abs=1e-7), name
            assert np.isfinite(grad).all() and not grad.any(), name


def test_cross_entropy_with_ignore_index_is_the_compaction():
    """the anchor: torch's own nn.CrossEntropyLoss(ignore_index=255) in float64 against the unmasked reference on the valid pixels"""
    case = T.Case("small_odd", 3)
    logits, onehot, valid = S.masked_inputs(case, "random30")
    index = torch.tensor(np.where(valid != 0, onehot.argmax(1), S.IGNORE)).long()
    x = torch.tensor(logits).double().requires_grad_()
    loss = nn.CrossEntropyLoss(ignore_index=S.IGNORE)(x, index)
    loss.backward()
    ref_loss, ref_grad = S.reference(case, "random30", "CrossEntropyLoss")
    assert abs(float(loss.detach()) - ref_loss) <= F64_BOUND and np.abs(x.grad.numpy() - ref_grad).max() <= F64_BOUND * np.abs(ref_grad).max()


@pytest.mark.parametrize("classes", (2, 3))
def test_mean_iou_and_dice_coefficient_with_a_mask(classes):
    from volume_segmantics_amd.data.losses import DiceCoefficient, MeanIoU, compute_per_channel_dice
    _x, probs, onehot, _ref = T.iou_inputs("small_odd", classes)
    case = T.Case("small_odd", classes)
    for pattern in ("random30", "sample_out", "one_pixel"):
        valid = S.valid_mask(case, pattern)
        got = float(MeanIoU()(probs, onehot, torch.tensor(valid)))
        assert abs(got - S.iou_reference(probs, onehot, valid)) <= T.IOU_BOUND, pattern
        dice = float(DiceCoefficient()(probs.double(), onehot, torch.tensor(valid)))
        want = compute_per_channel_dice(torch.tensor(S.compact(probs.double().numpy(), valid)), torch.tensor(S.compact(onehot.numpy(), valid)))
        assert abs(dice - float(want.mean())) <= F64_BOUND, pattern
    assert np.isnan(float(MeanIoU()(probs, onehot, torch.tensor(S.valid_mask(case, "none")))))
    assert np.isnan(float(MeanIoU().from_logits(_x, onehot, torch.tensor(S.valid_mask(case, "none")))))


# ---- slicer ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", (np.uint8, np.int32))
@pytest.mark.parametrize("ignore,classes", [(9, (0, 3, 7)), (5, (0, 3, 7)), (0, (2, 3, 7)), (255, (0, 1, 2)), (4, (0, 200)), (1, (0, 2))])
def test_slicer_relabels_around_the_ignore_value(ignore, classes, dtype):
    """ignore value above, inside and below the class values; two classes plus ignore is a binary run"""
    from volume_segmantics_amd.data import TrainingDataSlicer
    from volume_segmantics_amd.data.volume_feed import volumes_as_ubyte
    data, labels = S.sparse_volume(ignore, classes, dtype)
    slicer = TrainingDataSlicer(data, labels.copy(), _settings(ignore))
    want = np.full(labels.shape, S.IGNORE, np.uint8)
    for new, old in enumerate(sorted(classes)):
        want[labels == old] = new
    assert slicer.seg_vol.dtype == np.uint8 and np.array_equal(slicer.seg_vol, want)
    assert slicer.num_seg_classes == len(classes) and slicer.multilabel == (len(classes) > 2)
    assert slicer.codes == [f"label_val_{v}" for v in sorted(classes)] and slicer.ignore_seen
    assert np.array_equal(volumes_as_ubyte(slicer)[1], want)            # the binary clamp leaves 255 alone


def test_slicer_refusals():
    from volume_segmantics_amd.data import TrainingDataSlicer
    from volume_segmantics_amd.data.slicers import check_ignore_label_occurs
    from volume_segmantics_amd.data.volume_feed import build_sample_table
    data, labels = S.sparse_volume(9)
    with pytest.raises(ValueError, match="nothing but the ignore label"):
        TrainingDataSlicer(data, np.full_like(labels, 9), _settings(9))
    typo = [TrainingDataSlicer(data, labels.copy(), _settings(99)), TrainingDataSlicer(data, labels.copy(), _settings(99))]
    assert typo[0].num_seg_classes == 4                                  # (9 is a class of that run)
    with pytest.raises(ValueError, match="occurs in no label volume"):
        check_ignore_label_occurs(typo)
    with pytest.raises(ValueError, match="occurs in no label volume"):
        build_sample_table(typo, V.SIZE)
    full = np.where(labels == 9, 0, labels)                                                   # one volume without the value is fine ..
    check_ignore_label_occurs([TrainingDataSlicer(data, full, _settings(9)), TrainingDataSlicer(data, labels.copy(), _settings(9))])
    many = (np.arange(np.prod(S.SPARSE_SHAPE)).reshape(S.SPARSE_SHAPE) % 256).astype(np.uint8)   # 255 classes next to an ignore label
    with pytest.raises(ValueError, match="at most 254 classes"):
        TrainingDataSlicer(data, many, _settings(255))


@pytest.mark.parametrize("axes", ("All", "Z", "Y"))
def test_slices_without_a_label_are_left_out_on_both_routes(tmp_path, axes):
    """two labelled z-slices and one partly labelled row: the PNG route's files, the volume feed's samples and the definition agree,
    sample for sample, and the cut masks are the decoded PNGs"""
    from volume_segmantics_amd.data import TrainingDataSlicer
    from volume_segmantics_amd.data.volume_feed import build_sample_table, cut_numpy
    volumes = [S.sparse_volume(9, seed=0), S.sparse_volume(9, (0, 1), seed=1)]
    slicers = [TrainingDataSlicer(d, l.copy(), _settings(9, axes)) for d, l in volumes]
    images, masks = V.png_route_pairs(slicers, tmp_path)
    names = sorted((p.name for p in (tmp_path / "seg").glob("*.png")), key=lambda s: __import__("re").split(r"(\d+)", s))
    letters = "zyx" if axes == "All" else axes.lower()
    want = {f"seg{k}_{a}_stack_{i}.png" for k, (_d, l) in enumerate(volumes) for a in letters for i in S.kept_slices(l, 9)[a]}
    assert set(names) == want and len(want) == 2 * sum({"z": 3, "y": 10, "x": 8}[a] for a in letters)
    assert {p.name.replace("data", "seg") for p in (tmp_path / "data").glob("*.png")} == want
    table = build_sample_table(slicers, V.SIZE)
    assert len(table) == len(want) == len(masks) and table.ignore_label == S.IGNORE
    from volume_segmantics_amd.data.datasets import VolSeg2dDataset
    files = [p.name for p in VolSeg2dDataset(tmp_path / "data", tmp_path / "seg", V.SIZE, augment="device").masks_fps]
    assert files == [f"seg{k}_{a}_stack_{i}.png" for k, a, i in table.samples]
    cut_images, cut_masks = cut_numpy(table.store.data, table.store.labels, table.descriptors, V.SIZE)
    assert np.array_equal(cut_images, images) and np.array_equal(cut_masks, masks)
    assert set(np.unique(masks)) <= {0, 1, 2, S.IGNORE} and (masks == S.IGNORE).any()
    for j, (k, a, i) in enumerate(table.samples):
        assert (masks[j] != S.IGNORE).any(), (k, a, i)


def test_a_run_without_a_kept_slice_raises(tmp_path):
    from volume_segmantics_amd.data import TrainingDataSlicer
    from volume_segmantics_amd.data.volume_feed import build_sample_table
    data, labels = S.sparse_volume(9)
    slicer = TrainingDataSlicer(data, labels, _settings(9))
    slicer.seg_vol[:] = S.IGNORE                                          # (cannot be constructed: the slicer refuses such a volume)
    slicer._labelled.clear()
    with pytest.raises(ValueError, match="no slice"):
        build_sample_table([slicer], V.SIZE)
    with pytest.raises(ValueError, match="no slice"):
        slicer.output_label_slices(tmp_path / "seg", "seg0")


# ---- label-range checks ------------------------------------------------------------------------------------------------------------
class _Pairs(torch.utils.data.Dataset):
    def __init__(self, masks):
        self.masks = masks

    def __len__(self):
        return len(self.masks)

    def __getitem__(self, i):
        return torch.zeros((1,) + self.masks[i].shape, dtype=torch.uint8), torch.from_numpy(self.masks[i])


@pytest.mark.parametrize("bad", (None, 254, 3))
def test_range_checks_leave_255_out_and_still_raise(bad):
    """a 3-class run: 255 passes every check, a 254 (or a 3) raises the reference's text in all three places"""
    from volume_segmantics_amd.data import TrainingDataSlicer
    from volume_segmantics_amd.data.datasets import ResidentSliceLoader, ShardedBatchSampler
    from volume_segmantics_amd.data.volume_feed import VolumeSliceLoader, build_sample_table
    from volume_segmantics_amd.utilities.base_data_utils import prepare_training_batch
    data, labels = S.sparse_volume(9)
    slicer = TrainingDataSlicer(data, labels, _settings(9))
    if bad is not None:
        slicer.seg_vol[3, 2, 2] = bad
    table = build_sample_table([slicer], V.SIZE)
    sampler = ShardedBatchSampler(len(table), 4, shuffle=False, drop_last=False)
    volume_loader = VolumeSliceLoader(table, sampler, "cpu")
    masks = np.stack([m.numpy() for batch in volume_loader for m in batch[1]])
    resident = ResidentSliceLoader(_Pairs(masks), sampler, "cpu", ignore_label=S.IGNORE)
    assert (masks == S.IGNORE).any() and resident.max_label == volume_loader.max_label == (2 if bad is None else bad)
    batch = (torch.zeros((len(masks), 1, V.SIZE, V.SIZE)), torch.from_numpy(masks))
    for loader in (volume_loader, resident):
        loader.num_labels = 3
    if bad is None:
        assert len(list(volume_loader)) == len(list(resident)) == len(sampler)
        _inputs, targets, valid = prepare_training_batch(batch, "cpu", 3, ignore_label=S.IGNORE)
        assert targets.dtype == valid.dtype == torch.uint8 and targets.shape == (len(masks), 3, V.SIZE, V.SIZE)
        assert np.array_equal(valid.numpy(), masks != S.IGNORE)
        assert np.array_equal(targets.numpy(), (masks[:, None] == np.arange(3)[None, :, None, None]).astype(np.uint8))
        return
    for run in (lambda: list(volume_loader), lambda: list(resident), lambda: prepare_training_batch(batch, "cpu", 3, ignore_label=S.IGNORE)):
        with pytest.raises(RuntimeError, match="Class values must be smaller than num_classes."):
            run()


def test_too_many_classes_next_to_an_ignore_label():
    from volume_segmantics_amd.utilities.base_data_utils import prepare_training_batch
    batch = (torch.zeros((1, 1, 4, 4)), torch.zeros((1, 4, 4), dtype=torch.uint8))
    with pytest.raises(ValueError, match="at most 254 classes"):
        prepare_training_batch(batch, "cpu", 255, ignore_label=S.IGNORE)


# ---- augmentation ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("branch", list(S.augment_param_sets(64)))
def test_host_augmentation_keeps_mask_values(branch):
    """masks are resampled nearest-neighbour with reflect-101 borders: a mask over {0, 1, 255} stays within {0, 1, 255}"""
    from volume_segmantics_amd.data.augmentations import apply_params
    image, mask = S.sparse_mask_image(64)
    _image, out = apply_params(image, mask, S.augment_param_sets(64)[branch])
    assert out.shape == mask.shape and set(np.unique(out)) <= {0, 1, S.IGNORE}
    assert (out == S.IGNORE).any() and (out != S.IGNORE).any()


def test_host_augmentation_keeps_mask_values_over_random_draws():
    from volume_segmantics_amd.data.augmentations import train_augment
    image, mask = S.sparse_mask_image(64)
    rng = np.random.default_rng(11)
    for _ in range(24):
        assert set(np.unique(train_augment(image, mask, 64, rng)[1])) <= {0, 1, S.IGNORE}


# ---- without the key nothing changes -------------------------------------------------------------------------------------------------
def test_without_the_key_the_batch_is_a_pair():
    from volume_segmantics_amd.utilities.base_data_utils import prepare_training_batch
    masks = torch.from_numpy(np.random.default_rng(3).integers(0, 3, (2, 8, 8)).astype(np.uint8))
    out = prepare_training_batch((torch.zeros((2, 1, 8, 8)), masks), "cpu", 3)
    assert isinstance(out, tuple) and len(out) == 2
    assert torch.equal(out[1], torch.nn.functional.one_hot(masks.long(), 3).permute(0, 3, 1, 2).to(torch.uint8))
    with pytest.raises(RuntimeError, match="Class values"):
        prepare_training_batch((torch.zeros((2, 1, 8, 8)), masks + 253), "cpu", 3)


@pytest.mark.parametrize("variant", ("uint8_binary", "labels_0_255", "labels_0_3_7"))
def test_without_the_key_the_slicer_writes_every_slice_as_before(tmp_path, variant):
    """the key absent: every value is a class (255 included), every slice of every axis is written, and each label PNG holds the
    relabelled (binary: clamped) slice - stated here with np.unique, independently of the slicer"""
    from PIL import Image
    from volume_segmantics_amd.data import TrainingDataSlicer
    from volume_segmantics_amd.data.volume_feed import build_sample_table
    shape = (5, 6, 7)
    data, labels = V.volume_pair(shape, variant, 0)
    slicer = TrainingDataSlicer(data, labels.copy(), _settings())
    assert slicer.ignore_label is None and not slicer.ignore_seen
    values, inverse = np.unique(labels, return_inverse=True)
    want = inverse.reshape(shape).astype(np.uint8)
    assert slicer.num_seg_classes == len(values) and np.array_equal(slicer.seg_vol, want)
    V.write_pngs([slicer], tmp_path)
    files = sorted(p.name for p in (tmp_path / "seg").glob("*.png"))
    assert files == sorted(f"seg0_{a}_stack_{i}.png" for a, n in zip("zyx", shape) for i in range(n))
    for a, n in zip("zyx", shape):
        for i in range(n):
            got = np.array(Image.open(tmp_path / "seg" / f"seg0_{a}_stack_{i}.png"))
            assert np.array_equal(got, np.take(want, i, axis="zyx".index(a))), (a, i)
            got = np.array(Image.open(tmp_path / "data" / f"data0_{a}_stack_{i}.png"))
            assert np.array_equal(got, np.take(data, i, axis="zyx".index(a))), (a, i)
    table = build_sample_table([slicer], V.SIZE)
    assert len(table) == sum(shape) and table.ignore_label is None


def test_trainer_reads_the_key_once_and_declines_the_recorded_step(caplog):
    """host-side wiring: the mask reaches the criterion, and `step_mode: graph` with an ignore label takes the call-by-call step"""
    import logging
    from volume_segmantics_amd.model.operations.vol_seg_2d_trainer import VolSeg2dTrainer
    trainer = VolSeg2dTrainer.__new__(VolSeg2dTrainer)
    trainer.settings = SimpleNamespace(step_mode="graph", loss_criterion="BCELoss")
    trainer.ignore_label, trainer.label_no, trainer._graph_declined, trainer.world, trainer.rank = S.IGNORE, 2, False, 1, 0
    trainer.loss_criterion = nn.BCEWithLogitsLoss()
    fused = []

    class Model(nn.Module):
        def __init__(self):
            super().__init__()
            self.conv = nn.Conv2d(1, 2, 1)

        def forward(self, x):
            return self.conv(x)

        def can_fuse_step(self, *args):
            fused.append(args)
            return True

    trainer.model = Model()
    trainer.optimizer = torch.optim.SGD(trainer.model.parameters(), lr=0.1)
    scheduler = torch.optim.lr_scheduler.LambdaLR(trainer.optimizer, lambda _: 1.0)
    masks = torch.full((2, 8, 8), S.IGNORE, dtype=torch.uint8)
    masks[0, 2] = 1
    batch = (torch.randn(2, 1, 8, 8, generator=torch.Generator().manual_seed(0)), masks)
    with caplog.at_level(logging.INFO):
        first = trainer._train_one_batch(scheduler, batch)
        trainer._train_one_batch(scheduler, batch)
    assert not fused and sum("call by call" in r.message for r in caplog.records) == 1
    inputs, targets, valid = trainer._batch(batch)
    from volume_segmantics_amd.data.losses import masked_bce_with_logits
    assert int(valid.sum()) == 8 and torch.isfinite(first)
    masks[:] = S.IGNORE
    empty = trainer._train_one_batch(scheduler, (batch[0], masks))
    assert float(empty) == 0.0 and all(float(p.grad.abs().max()) == 0.0 for p in trainer.model.parameters())
    assert float(masked_bce_with_logits(trainer.model(inputs), targets, valid)) > 0.0
