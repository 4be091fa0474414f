"""TrainingDataSlicer - 3-D data / label volumes to 2-D PNG slices on disk for training
(reference: volume_segmantics/data/slicers.py:14-149).  Host-side data preparation next to the accelerated path: label classes
are made sequential from zero (:48-71), slices are written along z / y / x per ``training_axes`` as
``<prefix>_<axis>_stack_<index>.png`` (:100-118), volumes that are not uint8 go through skimage's ``img_as_ubyte`` (restated
below: scikit-image is not installed next to torch here) and binary labels are clamped to {0, 1} (:120-135)."""
from __future__ import annotations

import logging
import os
from pathlib import Path
from types import SimpleNamespace
from typing import Union

import numpy as np

from ..utilities import base_data_utils as utils
from .base_data_manager import BaseDataManager


def _scale_bits(a: np.ndarray, n: int, m: int) -> np.ndarray:
    """skimage.util.dtype._scale: integers of n significant bits to m bits (a copy)."""
    a = a.copy()
    if n > m:                       # downscale with precision loss
        a //= 2 ** (n - m)
        return a
    if n == m:
        return a
    if m % n == 0:                  # exact upscale: replicate the bit pattern
        a *= (2 ** m - 1) // (2 ** n - 1)
        return a
    o = (m // n + 1) * n            # upscale to a multiple of n bits, then down to m
    a = a.astype(np.int64 if a.dtype.kind == "i" else np.uint64)
    a *= (2 ** o - 1) // (2 ** n - 1)
    a //= 2 ** (o - m)
    return a


def img_as_ubyte(image: np.ndarray) -> np.ndarray:
    """skimage.img_as_ubyte (scikit-image 0.18 ``util.dtype._convert(image, np.uint8)``), restated; known answers from the real
    function are in tests/test_host_logic.py.  NOTE the behaviour the reference inherits: integers are RESCALED by bit depth, so
    an int64 / int32 / uint32 label volume with values 0..3 becomes all zeros and uint16 1000 becomes 3 - the reference's label
    volumes are uint8 in practice (HDF5 / TIFF), which pass through untouched."""
    image = np.asarray(image)
    dt = image.dtype
    if dt == np.uint8:
        return image
    if dt == np.bool_:
        return image.astype(np.uint8) * 255
    if dt.kind == "f":
        if image.size and (np.min(image) < -1.0 or np.max(image) > 1.0):
            raise ValueError("Images of type float must be between -1 and 1.")
        out = np.multiply(image, 255, dtype=np.float64 if dt.itemsize > 4 else np.float32)
        np.rint(out, out=out)
        np.clip(out, 0, 255, out=out)
        return out.astype(np.uint8)
    if dt.kind == "u":
        return _scale_bits(image, 8 * dt.itemsize, 8).astype(np.uint8)
    if dt.kind == "i":
        scaled = _scale_bits(image, 8 * dt.itemsize - 1, 8)
        return np.maximum(scaled, 0).astype(np.uint8)
    raise ValueError(f"img_as_ubyte: unsupported dtype {dt}")


def imsave_png(path: Union[str, Path], data: np.ndarray) -> None:
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(data)).save(str(path))


def clamp_binary_labels(labels: np.ndarray, sparse: bool = False) -> np.ndarray:
    """The reference's clamp of binary labels to {0, 1} (a copy); with sparse labels the unlabelled value 255 stays."""
    labels = labels.copy()
    if sparse:
        labels[(labels > 1) & (labels != utils.IGNORE_INDEX)] = 1
    else:
        labels[labels > 1] = 1
    return labels


def kept_slice_counts(slicer, axis_enum) -> dict:
    """{axis letter: slices kept} of one slicer's training axes, logged; a volume none of whose slices is kept is an error."""
    axes = "zyx" if axis_enum == utils.Axis.ALL else axis_enum.name.lower()
    counts = {axis: int(slicer.labelled_slices(axis).sum()) for axis in axes}
    shape = dict(zip("zyx", np.asarray(slicer.seg_vol).shape))
    logging.info("Slices with a labelled voxel, kept for training: " + ", ".join(f"{a}: {counts[a]} of {shape[a]}" for a in axes))
    if not sum(counts.values()):
        raise ValueError("no slice of the label volume holds a labelled voxel")
    return counts


def check_ignore_label_occurs(slicers) -> None:
    """An ``ignore_label`` that is in no label volume of the run is most likely a typo in the settings: refuse it."""
    slicers = list(slicers)
    ignore = {s.ignore_label for s in slicers}
    if len(ignore) != 1:
        raise ValueError("the slicers of one training run share their ignore_label")
    ignore = ignore.pop()
    if ignore is not None and not any(s.ignore_seen for s in slicers):
        raise ValueError(f"ignore_label {ignore} occurs in no label volume of this run")


class TrainingDataSlicer(BaseDataManager):
    """Image pre-processing (BaseDataManager) + slicing of the data and label volumes to PNG files in the xy (z), xz (y) and
    yz (x) planes."""

    def __init__(self, data_vol: Union[str, np.ndarray], label_vol: Union[str, np.ndarray], settings: SimpleNamespace):
        super().__init__(data_vol, settings)
        self.data_im_out_dir = None
        self.seg_im_out_dir = None
        self.multilabel = False
        self.settings = settings
        self.label_vol_path = utils.setup_path_if_exists(label_vol)
        if self.label_vol_path is not None:
            self.seg_vol, _ = utils.get_numpy_from_path(self.label_vol_path, internal_path=settings.seg_hdf5_path)
        elif isinstance(label_vol, np.ndarray):
            self.seg_vol = label_vol
        else:
            raise TypeError("label_vol must be a path or a numpy array")
        self._preprocess_labels()

    def _preprocess_labels(self):
        self.ignore_label = getattr(self.settings, "ignore_label", None)
        self.ignore_seen, self._labelled = False, {}
        if self.ignore_label is not None:
            self._preprocess_sparse_labels(int(self.ignore_label))
            return
        seg_classes = np.unique(self.seg_vol)
        self.num_seg_classes = len(seg_classes)
        if self.num_seg_classes > 2:
            self.multilabel = True
        logging.info(f"Number of classes in segmentation dataset: {self.num_seg_classes}")
        logging.info(f"These classes are: {seg_classes}")
        if seg_classes[0] != 0 or not utils.sequential_labels(seg_classes):
            logging.info("Fixing label classes.")
            self._fix_label_classes(seg_classes)
        self.codes = [f"label_val_{i}" for i in seg_classes]

    def _fix_label_classes(self, seg_classes):
        """Relabel so that the classes are 0 .. K-1 (ascending input order), in place as the reference does."""
        for idx, current in enumerate(seg_classes):
            self.seg_vol[self.seg_vol == current] = idx

    def _preprocess_sparse_labels(self, ignore: int):
        """Sparse labels (settings key ``ignore_label``): the classes are the distinct values other than ``ignore``, relabelled
        0 .. K-1 in ascending order; ``ignore`` becomes 255 (base_data_utils.IGNORE_INDEX).  The result is a new uint8 volume, so
        img_as_ubyte never rescales it, whatever the dtype of the input."""
        values = np.unique(self.seg_vol)
        seg_classes = values[values != ignore]
        self.ignore_seen = len(seg_classes) != len(values)
        if not len(seg_classes):
            raise ValueError(f"the label volume holds nothing but the ignore label {ignore}")
        if len(seg_classes) > 254:
            raise ValueError(f"{len(seg_classes)} classes and an ignore label: at most 254 classes fit next to the unlabelled "
                             f"value {utils.IGNORE_INDEX} in uint8 labels")
        self.num_seg_classes = len(seg_classes)
        self.multilabel = self.num_seg_classes > 2
        logging.info(f"Number of classes in segmentation dataset: {self.num_seg_classes} (ignore label {ignore} set aside)")
        logging.info(f"These classes are: {seg_classes}")
        relabelled = np.searchsorted(seg_classes, self.seg_vol).astype(np.uint8)     # (the ignore value lands anywhere: overwritten)
        relabelled[self.seg_vol == ignore] = utils.IGNORE_INDEX
        self.seg_vol = relabelled
        self.codes = [f"label_val_{i}" for i in seg_classes]

    @property
    def class_counts(self) -> np.ndarray:
        """Labelled voxels per relabelled class 0 .. K-1 (int64; the unlabelled value 255 of sparse labels is not counted): one
        np.bincount over the volume, taken when first asked for (``loss_class_weights: balanced``) and kept."""
        if getattr(self, "_class_counts", None) is None:
            flat = np.asarray(self.seg_vol).reshape(-1)
            if flat.dtype.kind not in "ui":
                flat = flat.astype(np.int64)
            counts = np.bincount(flat, minlength=self.num_seg_classes)
            if self.ignore_label is not None:
                counts = counts[:utils.IGNORE_INDEX]
            self._class_counts = counts[:self.num_seg_classes].astype(np.int64)
        return self._class_counts

    def labelled_slices(self, axis: str) -> np.ndarray:
        """Per slice along ``axis`` ('z', 'y', 'x'): whether it holds a value other than 255.  All true without an ignore label."""
        n = self.seg_vol.shape["zyx".index(axis)]
        if self.ignore_label is None:
            return np.ones(n, dtype=bool)
        if axis not in self._labelled:
            others = tuple(a for a in range(3) if a != "zyx".index(axis))
            self._labelled[axis] = (np.asarray(self.seg_vol) != utils.IGNORE_INDEX).any(axis=others)
        return self._labelled[axis]

    def output_data_slices(self, data_dir: Path, prefix: str) -> None:
        self.data_im_out_dir = Path(data_dir)
        logging.info("Slicing data volume and saving slices to disk")
        os.makedirs(data_dir, exist_ok=True)
        self._output_slices_to_disk(self.data_vol, Path(data_dir), prefix)

    def output_label_slices(self, data_dir: Path, prefix: str) -> None:
        self.seg_im_out_dir = Path(data_dir)
        logging.info("Slicing label volume and saving slices to disk")
        os.makedirs(data_dir, exist_ok=True)
        self._output_slices_to_disk(self.seg_vol, Path(data_dir), prefix, label=True)

    def _output_slices_to_disk(self, data_arr, output_path, name_prefix, label=False):
        axis_enum = utils.get_training_axis(self.settings)
        if self.ignore_label is not None:
            kept_slice_counts(self, axis_enum)      # logs the slices kept per axis, raises when there is none
        for axis, index in utils.get_axis_index_pairs(data_arr.shape, axis_enum):
            if self.ignore_label is not None and not self.labelled_slices(axis)[index]:      # sparse labels: a slice without a labelled voxel is left out of the run
                continue
            self._output_im(utils.axis_index_to_slice(data_arr, axis, index), output_path / f"{name_prefix}_{axis}_stack_{index}", label)

    def _output_im(self, data, path, label=False):
        if data.dtype != np.uint8:
            data = img_as_ubyte(data)
        if label and not self.multilabel:
            data = clamp_binary_labels(data, self.ignore_label is not None)
        imsave_png(f"{path}.png", data)

    def _delete_image_dir(self, im_dir_path):
        if im_dir_path is not None and Path(im_dir_path).exists():
            ims = list(Path(im_dir_path).glob("*.png"))
            logging.info(f"Deleting {len(ims)} images.")
            for im in ims:
                im.unlink()
            logging.info("Deleting the empty directory.")
            Path(im_dir_path).rmdir()

    def clean_up_slices(self) -> None:
        """Deletes data and label image slices created by the slicer."""
        self._delete_image_dir(self.data_im_out_dir)
        self._delete_image_dir(self.seg_im_out_dir)
