"""Shared by tests/test_volume_feed_host.py and tests/test_hip_volume_feed.py: the small volumes that take the slice cut of the
volume feed (data/volume_feed.py, csrc/slice_feed.hip) through every branch at image_size 32, and the PNG route's answer for them.

Shapes (depth, height, width):
    (7, 20, 32)   z: 20 x 32, no scaling, pad 6;  y: 7 x 32, no scaling, pad 12 / 13 rows around 7 - wider than the slice, several
                  reflections;  x: 7 x 20 scaled UP to 11 x 32
    (40, 48, 9)   every slice scaled DOWN (z 48 x 9 -> 32 x 6, y 40 x 9 -> 32 x 7, x 40 x 48 -> 27 x 32)
    (1, 16, 16)   one-row slices (1 x 16 -> 2 x 32) and a single 16 x 16 -> 32 x 32
    (1, 32, 20)   one-row slices that are NOT scaled (1 x 32): fit_to_square's "edge" border, which needs a fitted side of 1"""
from types import SimpleNamespace

import numpy as np

SIZE = 32
SHAPES = ((7, 20, 32), (40, 48, 9), (1, 16, 16), (1, 32, 20))
VARIANTS = ("uint8_binary", "float_data", "labels_0_255", "labels_0_3_7", "three_classes")


def settings(axes="All", **extra):
    return SimpleNamespace(st_dev_factor=2.575, downsample=False, clip_data=False, data_hdf5_path="/data", seg_hdf5_path="/data",
                           training_axes=axes, image_size=SIZE, **extra)


def volume_pair(shape, variant: str, seed: int):
    rng = np.random.default_rng([seed, VARIANTS.index(variant)])
    data = rng.integers(0, 256, size=shape, dtype=np.uint8)
    if variant == "float_data":      # float in [0, 1], not clipped: img_as_ubyte's rint(255 x)
        data = rng.random(shape, dtype=np.float32)
    classes = {"labels_0_255": (0, 255), "labels_0_3_7": (0, 3, 7), "three_classes": (0, 1, 2)}.get(variant, (0, 1))
    labels = np.asarray(classes, dtype=np.uint8)[rng.integers(0, len(classes), size=shape)]
    labels.reshape(-1)[:len(classes)] = classes      # every class present, whatever the draw
    return data, labels


def make_slicers(variant: str, shapes=SHAPES, axes="All"):
    from volume_segmantics_amd.data import TrainingDataSlicer
    return [TrainingDataSlicer(*volume_pair(shape, variant, seed), settings(axes)) for seed, shape in enumerate(shapes)]


def write_pngs(slicers, root):
    """The train command's PNG route: data<k> / seg<k> prefixes into one data and one label directory."""
    for count, slicer in enumerate(slicers):
        slicer.output_data_slices(root / "data", f"data{count}")
        slicer.output_label_slices(root / "seg", f"seg{count}")
    return root / "data", root / "seg"


def png_route_pairs(slicers, root, size=SIZE):
    """(images, masks), (n, size, size) uint8 each: VolSeg2dDataset(augment="device")[i] for every i of the PNG route."""
    from volume_segmantics_amd.data.datasets import VolSeg2dDataset
    ds = VolSeg2dDataset(*write_pngs(slicers, root), size, augment="device")
    pairs = [ds[i] for i in range(len(ds))]
    return np.stack([p[0][0].numpy() for p in pairs]), np.stack([p[1].numpy() for p in pairs])
