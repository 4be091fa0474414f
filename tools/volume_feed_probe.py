"""What the volume feed (data/volume_feed.py, csrc/slice_feed.hip) costs and saves, on the 256^3 vessels case of
tests/test_hip_config0_vessels.py (needs a GPU; prints the table profiles/volume_feed.txt keeps):

  1. time from the two HDF5 files to the first training batch on the device, both routes in one process: the PNG route (slice,
     write 1 536 PNGs, decode, fit, upload) and the volume route (convert, upload, cut), with the bytes each feed keeps resident;
  2. the cut kernel's time per batch of 32 slices of 256^2 drawn from one axis only - z (rows contiguous), y (rows a plane apart)
     and x (one byte per cache line) - and from a shuffled mix, next to the whole training step of the same run (bf16 U-Net /
     resnet34, batch 32, device-side augmentation, volume feed).
    python tools/volume_feed_probe.py [batch=32] [repeats=200]"""
import pathlib
import shutil
import sys
import tempfile
import time

REPO = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
import numpy as np
import torch

from volume_segmantics_amd.data import TrainingDataSlicer, get_settings_data
from volume_segmantics_amd.data import datasets, volume_feed
from volume_segmantics_amd.model.operations.vol_seg_2d_trainer import VolSeg2dTrainer
from volume_segmantics_amd.utilities import base_data_utils as utils

LABELS = REPO / "tests" / "golden" / "vessels_256cube_LABELS.h5"


def synthetic_data_from(labels01: np.ndarray, seed: int = 1234) -> np.ndarray:
    """The float32 data volume tests/test_hip_config0_vessels.py synthesises from the vessels labels (the same recipe and seed)."""
    rng = np.random.default_rng(seed)
    v = labels01.astype(np.float32)
    for _ in range(2):
        for ax in range(3):
            v = (np.roll(v, 1, ax) + 2 * v + np.roll(v, -1, ax)) / 4
    noise = rng.standard_normal(v.shape).astype(np.float32)
    for ax in range(3):
        noise = (np.roll(noise, 1, ax) + noise + np.roll(noise, -1, ax)) / 3
    return (1500.0 + 900.0 * v + 450.0 * noise).astype(np.float32)


def first_batch(route, data_path, settings, root):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    slicer = TrainingDataSlicer(data_path, LABELS, settings)
    t1 = time.perf_counter()
    if route == "png":
        slicer.output_data_slices(root / "data", "data0")
        slicer.output_label_slices(root / "seg", "seg0")
        t2 = time.perf_counter()
        train, _valid = datasets.get_2d_training_dataloaders(root / "data", root / "seg", settings)
        resident = sum(l.images.numel() + l.masks.numel() for l in (train, _valid))
    else:
        t2 = time.perf_counter()
        train, _valid = volume_feed.get_volume_training_loaders([slicer], settings)
        resident = train.table.store.nbytes + train.rows.numel() + _valid.rows.numel()
    images, masks = next(iter(train))
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    assert images.is_cuda and images.shape == (settings.batch_size, 1, 256, 256)
    print(f"  {route:6s} route: {t3 - t0:7.2f} s to the first batch on the device  (read + pre-process the volumes {t1 - t0:.2f} s, "
          f"write PNGs {t2 - t1:.2f} s, build the loaders + first batch {t3 - t2:.2f} s); resident {resident / 2**20:.1f} MiB")
    return slicer, (train, _valid)


def kernel_times(table, batch, repeats):
    dev = torch.device("cuda", 0)
    data, labels = table.store.on(dev)
    rows = torch.from_numpy(np.ascontiguousarray(table.descriptors).view(np.uint8).reshape(len(table), 64).copy()).to(dev)
    rng = np.random.default_rng(0)
    picks = {a: [i for i, (_k, ax, _i) in enumerate(table.samples) if ax == a] for a in "zyx"}
    picks["mixed"] = list(range(len(table)))
    for name, pool in picks.items():
        batches = [rows.index_select(0, torch.as_tensor(rng.choice(pool, batch, replace=False), device=dev)) for _ in range(8)]
        for b in batches:
            volume_feed.cut_device(data, labels, b, table.image_size)
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for r in range(repeats):
            volume_feed.cut_device(data, labels, batches[r % 8], table.image_size)
        stop.record()
        torch.cuda.synchronize()
        print(f"  cut kernel, {batch} slices of 256^2, {name:5s}: {start.elapsed_time(stop) / repeats * 1e3:8.1f} us per batch "
              f"(events around {repeats} launches, output allocation included)")


def step_time(slicer, settings, batch):
    trainer = VolSeg2dTrainer.from_volumes([slicer], slicer.num_seg_classes, settings)
    trainer._create_model_and_optimiser(1e-4, frozen=False)
    sched = trainer._create_oc_lr_scheduler(50, 1e-4)
    trainer.model.train()
    times = []
    for epoch in range(4):
        trainer._set_epoch(epoch)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = 0
        for b in trainer.training_loader:
            trainer._train_one_batch(sched, b)
            n += 1
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) / n)
    print(f"  whole training step (volume feed -> augment -> forward / backward / AdamW), batch {batch}: {min(times[1:]) * 1e3:.3f} ms "
          f"(best of 3 passes over {n} steps after a warm-up pass)")


def main():
    batch = int(sys.argv[1]) if len(sys.argv) > 1 else 32
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    root = pathlib.Path(tempfile.mkdtemp(prefix="volseg_feed_"))
    try:
        labels, _ = utils.numpy_from_hdf5(LABELS, "/data")
        data_path = root / "vessels_256cube_DATA.h5"
        utils.save_data_to_hdf5(synthetic_data_from((labels == 255).astype(np.uint8)), data_path, internal_path="/data")
        settings = get_settings_data(REPO / "volseg-settings" / "2d_model_train_settings.yaml")
        settings.model = dict(settings.model, encoder_weights=None)
        settings.clip_data, settings.precision, settings.batch_size = True, "bf16", batch
        torch.zeros(1, device="cuda").item()
        TrainingDataSlicer(data_path, LABELS, settings)          # warm-up: file cache, HIP module load, the pre-processing kernels
        print(f"HDF5 files -> first training batch on the device, 256^3 vessels case, {sum(labels.shape)} slice pairs, batch {batch}:")
        slicer, loaders = first_batch("volume", data_path, settings, root)
        table = volume_feed.build_sample_table([slicer], settings.image_size)
        del loaders
        first_batch("png", data_path, settings, root)
        kernel_times(table, batch, repeats)
        step_time(slicer, settings, batch)
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
