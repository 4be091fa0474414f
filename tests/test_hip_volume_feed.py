"""-m gpu: the volume feed on the MI355X - csrc/slice_feed.hip (vs_slices_cut_u8) against this repository's own PNG route, bit for
bit: the kernel alone, VolumeSliceLoader against ResidentSliceLoader, VolSeg2dTrainer.from_volumes against the PNG-directory
trainer, and the two commands in fresh child processes (each under its own time limit)."""
import subprocess
import sys
from datetime import date
from pathlib import Path

import numpy as np
import pytest
import torch

from hip_helpers import DEV
from volume_feed_cases import SIZE, VARIANTS, make_slicers, png_route_pairs, settings, write_pngs

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parents[1]
SEED = 20240611


def _rows(table, indices=None):
    from volume_segmantics_amd.data.volume_feed import CUT_DTYPE
    d = table.descriptors if indices is None else table.descriptors[np.asarray(indices, dtype=np.int64)]
    return torch.from_numpy(np.ascontiguousarray(d).view(np.uint8).reshape(len(d), CUT_DTYPE.itemsize).copy()).to(DEV)


def _assert_same(got, want, table, order=None):
    """Bit equality, naming the first sample and pixels that differ."""
    got = got.cpu().numpy()
    if np.array_equal(got, want):
        return
    bad = np.flatnonzero((got != want).reshape(len(got), -1).any(axis=1))
    j = int(bad[0])
    ys, xs = np.nonzero(got[j] != want[j])
    i = j if order is None else order[j]
    raise AssertionError(f"{len(bad)} of {len(got)} samples differ; first: batch slot {j} = sample {i} {table.samples[i]} {table.descriptors[i]}: "
                         f"{len(ys)} pixels, e.g. (y, x, got, want) " + str([(int(y), int(x), int(got[j, y, x]), int(want[j, y, x]))
                                                                            for y, x in list(zip(ys, xs))[:8]]))


@pytest.mark.parametrize("variant", VARIANTS)
def test_cut_kernel_equals_the_png_route_bit_for_bit(tmp_path, variant):
    from volume_segmantics_amd.data.volume_feed import CUT_DTYPE, build_sample_table, cut_device
    assert CUT_DTYPE.itemsize == 64       # sizeof(vs_slice_cut)
    want_images, want_masks = png_route_pairs(make_slicers(variant), tmp_path)
    table = build_sample_table(make_slicers(variant), SIZE)
    data, labels = table.store.on(DEV)
    images, masks = cut_device(data, labels, _rows(table), SIZE)            # every slice of every volume and axis in one launch
    torch.cuda.synchronize()
    assert images.shape == masks.shape == (len(table), SIZE, SIZE) and images.dtype == masks.dtype == torch.uint8
    _assert_same(masks, want_masks, table)
    _assert_same(images, want_images, table)
    # one shuffled batch across all volumes and axes, two samples twice
    order = np.random.default_rng(5).permutation(len(table))[:40].tolist()
    order[7], order[33] = order[2], order[20]
    picked = [table.samples[i] for i in order]
    assert {k for k, _a, _i in picked} == set(range(len(table.store.shapes))) and {a for _k, a, _i in picked} == {"z", "y", "x"}
    images, masks = cut_device(data, labels, _rows(table, order), SIZE)
    _assert_same(masks, want_masks[order], table, order)
    _assert_same(images, want_images[order], table, order)


def test_cut_entry_refuses_bad_arguments():
    from volume_segmantics_amd import _lib
    buf = torch.zeros(64, dtype=torch.uint8, device=DEV)
    assert _lib.lib.vs_slices_cut_u8(_lib.ptr(buf), 64, _lib.ptr(buf), 64, _lib.ptr(buf), 1, 30, _lib.ptr(buf), _lib.ptr(buf), None) != 0
    assert "multiple of 4" in _lib.last_error()
    assert _lib.lib.vs_slices_cut_u8(_lib.ptr(buf), 64, None, 64, _lib.ptr(buf), 1, 32, _lib.ptr(buf), _lib.ptr(buf), None) != 0
    assert "null pointer" in _lib.last_error()
    odd = torch.zeros(128, dtype=torch.uint8, device=DEV)[4:]
    assert _lib.lib.vs_slices_cut_u8(_lib.ptr(buf), 64, _lib.ptr(buf), 64, _lib.ptr(odd), 1, 32, _lib.ptr(buf), _lib.ptr(buf), None) != 0
    assert "8-byte aligned" in _lib.last_error()


def _loader_settings(**extra):
    return settings(batch_size=4, training_set_proportion=0.7, cuda_device=0, **extra)


def test_volume_loader_yields_the_resident_loaders_batches(tmp_path, monkeypatch):
    """Through both factories with one shared split seed: 96 slices of a (24, 32, 40) volume, 67 for training (16 batches of 4,
    drop_last) and 29 for validation (7 batches of 4 and a last one of 1)."""
    from volume_segmantics_amd.data import datasets, volume_feed
    monkeypatch.setattr(datasets, "shared_seed", lambda rank, world: SEED)
    monkeypatch.setattr(volume_feed, "shared_seed", lambda rank, world: SEED)
    slicers = make_slicers("three_classes", shapes=((24, 32, 40),))
    data_dir, seg_dir = write_pngs(slicers, tmp_path)
    png_train, png_valid = datasets.get_2d_training_dataloaders(data_dir, seg_dir, _loader_settings())
    vol_train, vol_valid = volume_feed.get_volume_training_loaders(make_slicers("three_classes", shapes=((24, 32, 40),)), _loader_settings())
    assert isinstance(png_train, datasets.ResidentSliceLoader) and isinstance(vol_train, volume_feed.VolumeSliceLoader)
    assert len(vol_train) == len(png_train) == 16 and len(vol_valid) == len(png_valid) == 8
    assert vol_train.data.data_ptr() == vol_valid.data.data_ptr()            # the volumes are resident once
    assert vol_train.table.nbytes < 2 * 24 * 32 * 40 + 64 * 96 + 1 and vol_train.max_label == png_train.max_label == 2
    for epoch in range(2):
        for loader in (png_train, vol_train):
            loader.batch_sampler.set_epoch(epoch)
        got, want = list(vol_train), list(png_train)
        assert len(got) == len(want) == 16
        for (gi, gm), (wi, wm) in zip(got, want):
            assert gi.shape == wi.shape == (4, 1, SIZE, SIZE) and gm.shape == wm.shape == (4, SIZE, SIZE)
            assert gi.is_cuda and gi.dtype == gm.dtype == torch.uint8
            assert torch.equal(gi, wi) and torch.equal(gm, wm)
        if epoch:
            assert not torch.equal(got[0][0], first)                            # set_epoch reshuffles
        first = got[0][0]
    got, want = list(vol_valid), list(png_valid)
    assert [g[0].shape[0] for g in got] == [w[0].shape[0] for w in want] == [4] * 7 + [1]
    assert all(torch.equal(g[0], w[0]) and torch.equal(g[1], w[1]) for g, w in zip(got, want))
    for loader in (png_train, vol_train, vol_valid):
        loader.num_labels = 2
        with pytest.raises(RuntimeError) as e:
            next(iter(loader))
        assert str(e.value) == "Class values must be smaller than num_classes."


def _synthetic_pair(cube=64, seed=3):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((cube,) * 3).astype(np.float32)
    for _ in range(3):
        for ax in range(3):
            v = (np.roll(v, 1, ax) + 2 * v + np.roll(v, -1, ax)) / 4
    labels = (v > np.percentile(v, 65)).astype(np.uint8)
    noisy = v / np.abs(v).max() * 90 + 128 + rng.standard_normal(v.shape) * 8
    return np.clip(noisy, 0, 255).astype(np.uint8), labels


def _train_settings(**extra):
    from volume_segmantics_amd.data import get_settings_data
    s = get_settings_data(REPO / "volseg-settings" / "2d_model_train_settings.yaml")
    s.image_size, s.precision = 64, "fp32"
    s.model = dict(s.model, encoder_weights=None)
    for k, v in extra.items():
        setattr(s, k, v)
    return s


def test_from_volumes_trains_exactly_as_the_png_directory_trainer(tmp_path, monkeypatch):
    from volume_segmantics_amd.data import TrainingDataSlicer, datasets, volume_feed
    from volume_segmantics_amd.model.model_2d import create_model_from_file
    from volume_segmantics_amd.model.operations.vol_seg_2d_trainer import VolSeg2dTrainer
    monkeypatch.setattr(datasets, "shared_seed", lambda rank, world: SEED)
    monkeypatch.setattr(volume_feed, "shared_seed", lambda rank, world: SEED)
    data, labels = _synthetic_pair()
    losses = {}
    for route in ("png", "volume"):
        s = _train_settings()
        assert s.model["type"] == "U_Net" and s.model["encoder_name"] == "resnet34"
        slicer = TrainingDataSlicer(data.copy(), labels.copy(), s)
        torch.manual_seed(11)
        if route == "png":
            slicer.output_data_slices(tmp_path / "data", "data0")
            slicer.output_label_slices(tmp_path / "seg", "seg0")
            trainer = VolSeg2dTrainer(tmp_path / "data", tmp_path / "seg", slicer.num_seg_classes, s)
            assert isinstance(trainer.training_loader, datasets.ResidentSliceLoader)
        else:
            trainer = VolSeg2dTrainer.from_volumes([slicer], slicer.num_seg_classes, s)
            assert isinstance(trainer.training_loader, volume_feed.VolumeSliceLoader)
        assert len(trainer.training_loader) == int(192 * 0.8) // 12
        out = tmp_path / f"{route}_model.pytorch"
        trainer.train_model(out, 1, s.patience, create=True, frozen=True)
        losses[route] = (list(trainer.avg_train_losses), list(trainer.avg_valid_losses))
        print(f"[volume feed] {route}: train {trainer.avg_train_losses}, valid {trainer.avg_valid_losses}")
        del trainer
    assert len(losses["png"][0]) == 1 and np.isfinite(losses["png"][0][0]) and np.isfinite(losses["png"][1][0])
    assert losses["volume"] == losses["png"]
    model, num_labels, _codes = create_model_from_file(tmp_path / "volume_model.pytorch")
    assert num_labels == 2 and sum(p.numel() for p in model.parameters()) > 2e7


def _run(cmd, limit):
    return subprocess.run([sys.executable, "-m"] + [str(c) for c in cmd], cwd=REPO, capture_output=True, text=True, timeout=limit)


@pytest.mark.parametrize("feed", ["volume", "png"])
def test_train_and_predict_commands(tmp_path, feed):
    import yaml
    from volume_segmantics_amd.utilities import base_data_utils as utils
    from volume_segmantics_amd.utilities import hdf5_lite
    assert utils._h5py() is not None or hdf5_lite.available(), "the commands read and write HDF5: h5py or libhdf5 is needed"
    data, labels = _synthetic_pair()
    data_path, label_path = tmp_path / "blobs_DATA.h5", tmp_path / "blobs_LABELS.h5"
    utils.save_data_to_hdf5(data, data_path, internal_path="/data")
    utils.save_data_to_hdf5(labels, label_path, internal_path="/data")
    (tmp_path / "volseg-settings").mkdir()
    train = yaml.safe_load((REPO / "volseg-settings" / "2d_model_train_settings.yaml").read_text())
    train.update(image_size=64, num_cyc_frozen=1, num_cyc_unfrozen=0, slice_feed=feed)
    train["model"]["encoder_weights"] = None
    (tmp_path / "volseg-settings" / "2d_model_train_settings.yaml").write_text(yaml.safe_dump(train))
    (tmp_path / "volseg-settings" / "2d_model_predict_settings.yaml").write_text(
        (REPO / "volseg-settings" / "2d_model_predict_settings.yaml").read_text())
    done = _run(["volume_segmantics_amd.scripts.train_2d_model", "--data", data_path, "--labels", label_path, "--data_dir", tmp_path], 300)
    assert done.returncode == 0, done.stderr[-3000:]
    model = tmp_path / f"{date.today()}_U_NET_trained_2d_model.pytorch"
    assert model.exists() and (tmp_path / f"{model.stem}_train_stats.csv").exists()
    assert not (tmp_path / "data").exists() and not (tmp_path / "seg").exists()
    if feed == "png":           # written, used and removed
        assert "Slicing data volume and saving slices to disk" in done.stderr and done.stderr.count("Deleting 192 images.") == 2
        return
    assert "Slicing data volume" not in done.stderr and "Deleting" not in done.stderr          # no slice was written
    done = _run(["volume_segmantics_amd.scripts.predict_2d_model", model, data_path, "--data_dir", tmp_path], 300)
    assert done.returncode == 0, done.stderr[-3000:]
    pred, _chunks = utils.numpy_from_hdf5(tmp_path / f"{date.today()}_blobs_DATA_2d_model_vol_pred.h5", "/data")
    assert pred.shape == data.shape and pred.dtype == np.uint8 and int(pred.max()) <= 1
