"""The training feed straight from the volumes: no PNG slices on disk, no fitted copies of the volume per axis in HBM.

The PNG route (slicers.TrainingDataSlicer -> datasets.VolSeg2dDataset -> datasets.ResidentSliceLoader) writes every slice of every
axis as a PNG, decodes it again, fits it to the square training size and keeps the fitted pairs.  Here the uint8 data and label
volumes are uploaded ONCE and a batch is one launch of csrc/slice_feed.hip (vs_slices_cut_u8), which cuts the fitted pairs out of
the volumes through a table of per-sample descriptors - the very bytes the PNG route's ``VolSeg2dDataset(augment="device")[i]``
holds for the same ``i`` (tests/test_volume_feed_host.py, tests/test_hip_volume_feed.py).

    table = build_sample_table(slicers, image_size)        # sample i = PNG-route dataset index i
    loader = VolumeSliceLoader(table.subset(indices), batch_sampler, device)
    get_volume_training_loaders(slicers, settings, rank, world)      # the 80/20 split + samplers of get_2d_training_dataloaders

``cut_numpy`` is the NumPy form of the kernel's arithmetic: it feeds CPU devices and states the cut independently of the
kernel and of datasets.fit_to_square (index maps per output pixel instead of resize + np.pad on whole images)."""
from __future__ import annotations

import logging

import numpy as np
import torch

from ..utilities import base_data_utils as utils
from .datasets import ShardedBatchSampler, natsort_key, shared_seed
from .slicers import check_ignore_label_occurs, clamp_binary_labels, img_as_ubyte, kept_slice_counts

# vs_slice_cut (include/volseg_hip.h), field for field
CUT_DTYPE = np.dtype([("img_off", "<i8"), ("msk_off", "<i8"), ("row_stride", "<i8"), ("col_stride", "<i8"), ("h", "<i4"), ("w", "<i4"),
                      ("nh", "<i4"), ("nw", "<i4"), ("top", "<i4"), ("left", "<i4"), ("border", "<i4"), ("reserved", "<i4")])
BORDER_REFLECT, BORDER_EDGE = 0, 1
_SCAN_CHUNK = 256        # samples per launch of the label-range scan: 32 MiB of temporary pairs at 256^2, 128 MiB at 512^2


def slice_file_stem(prefix: str, axis: str, index: int) -> str:
    """The name TrainingDataSlicer gives a slice (slicers.py:_output_slices_to_disk), without the suffix."""
    return f"{prefix}_{axis}_stack_{index}"


def sample_order(shapes, axis_enum, prefix: str = "data", keep=None):
    """[(volume, axis letter, index)] in the order the PNG route numbers its samples: VolSeg2dDataset sorts the file names
    ``<prefix><volume>_<axis>_stack_<index>.png`` with natsort_key, so the same names are built and sorted with the same key here.
    ``keep`` (sparse labels): per volume a function axis letter -> bool per slice (TrainingDataSlicer.labelled_slices); a slice
    that is not kept has no PNG files and no sample - the names and the order of the others do not change."""
    named = []
    for k, shape in enumerate(shapes):
        for axis, index in utils.get_axis_index_pairs(shape, axis_enum):
            if keep is not None and not keep[k](axis)[index]:
                continue
            named.append((natsort_key(slice_file_stem(f"{prefix}{k}", axis, index) + ".png"), k, axis, index))
    named.sort(key=lambda t: t[0])
    return [(k, axis, index) for _key, k, axis, index in named]


def fitted_geometry(h: int, w: int, size: int):
    """(nh, nw, top, left, border) of datasets.fit_to_square for an (h, w) slice, with its own expressions."""
    scale = size / max(h, w)
    if scale != 1.0:
        nh, nw = max(1, int(round(h * scale))), max(1, int(round(w * scale)))
    else:
        nh, nw = h, w
    if nh > size or nw > size:
        raise ValueError(f"a {h} x {w} slice does not fit image_size {size}")
    top, left = (size - nh) // 2, (size - nw) // 2
    return nh, nw, top, left, (BORDER_REFLECT if min(nh, nw) > 1 else BORDER_EDGE)


def volumes_as_ubyte(slicer):
    """(data, labels) of a TrainingDataSlicer as the uint8 volumes its PNG slices are cut from: element-wise what
    TrainingDataSlicer._output_im does to every slice - img_as_ubyte for anything that is not uint8 (the same errors), binary
    labels clamped to {0, 1}; the relabelling to 0 .. K-1 was done by the slicer already."""
    data, seg = np.asarray(slicer.data_vol), np.asarray(slicer.seg_vol)
    if data.ndim != 3 or seg.ndim != 3:
        raise ValueError("the volume feed takes 3-D data and label volumes")
    if data.shape != seg.shape:
        raise ValueError(f"data volume {data.shape} and label volume {seg.shape} differ in shape")
    if data.dtype != np.uint8:
        data = img_as_ubyte(data)
    if seg.dtype != np.uint8:
        seg = img_as_ubyte(seg)
    if not slicer.multilabel:
        seg = clamp_binary_labels(seg, getattr(slicer, "ignore_label", None) is not None)
    return np.ascontiguousarray(data), np.ascontiguousarray(seg)


class _VolumeStore:
    """The volumes of a table, concatenated: one data buffer, one label buffer; on a device once, shared by every subset."""

    def __init__(self, data_vols, label_vols):
        self.shapes = [v.shape for v in data_vols]
        self.bases = np.concatenate([[0], np.cumsum([v.size for v in data_vols])]).astype(np.int64)
        self.data, self.labels = self._flat(data_vols), self._flat(label_vols)
        self._resident = {}

    @staticmethod
    def _flat(vols) -> np.ndarray:
        if len(vols) == 1:      # the usual case: no second host copy
            return vols[0].reshape(-1)
        return np.concatenate([v.reshape(-1) for v in vols]) if vols else np.empty(0, np.uint8)

    @property
    def nbytes(self) -> int:
        return int(self.data.size + self.labels.size)

    def on(self, device):
        device = torch.device(device)
        if device not in self._resident:
            self._resident[device] = (torch.from_numpy(self.data).to(device), torch.from_numpy(self.labels).to(device))
        return self._resident[device]


class VolumeSampleTable:
    """Samples (volume, axis, index) over a shared _VolumeStore, with one vs_slice_cut descriptor each."""

    def __init__(self, store: _VolumeStore, samples, image_size: int, descriptors: np.ndarray | None = None):
        self.store, self.samples, self.image_size = store, list(samples), int(image_size)
        self.ignore_label = None      # 255 when the label volumes are sparse (build_sample_table): left out of the label-range check
        self.descriptors = self._describe() if descriptors is None else descriptors

    def __len__(self):
        return len(self.samples)

    @property
    def nbytes(self) -> int:
        """Device memory the feed keeps: the two volume buffers and the table."""
        return self.store.nbytes + int(self.descriptors.nbytes)

    def subset(self, indices) -> "VolumeSampleTable":
        indices = [int(i) for i in indices]
        part = VolumeSampleTable(self.store, [self.samples[i] for i in indices], self.image_size,
                                 self.descriptors[np.asarray(indices, dtype=np.int64)])
        part.ignore_label = self.ignore_label
        return part

    def _describe(self) -> np.ndarray:
        d = np.zeros(len(self.samples), dtype=CUT_DTYPE)
        for j, (k, axis, index) in enumerate(self.samples):
            depth, height, width = self.store.shapes[k]
            if axis == "z":       # vol[index]: (height, width)
                n, off, rs, cs, h, w = depth, index * height * width, width, 1, height, width
            elif axis == "y":     # vol[:, index]: (depth, width)
                n, off, rs, cs, h, w = height, index * width, height * width, 1, depth, width
            elif axis == "x":     # vol[:, :, index]: (depth, height)
                n, off, rs, cs, h, w = width, index, height * width, width, depth, height
            else:
                raise ValueError(f"unknown axis {axis!r}")
            if not 0 <= index < n:
                raise IndexError(f"slice {index} of axis {axis} of a volume of shape {self.store.shapes[k]}")
            base = int(self.store.bases[k])
            nh, nw, top, left, border = fitted_geometry(h, w, self.image_size)
            d[j] = (base + off, base + off, rs, cs, h, w, nh, nw, top, left, border, 0)
        last = d["img_off"] + (d["h"].astype(np.int64) - 1) * d["row_stride"] + (d["w"].astype(np.int64) - 1) * d["col_stride"]
        if len(d) and (d["img_off"].min() < 0 or last.max() >= self.store.data.size):
            raise IndexError("sample table addresses voxels outside its volumes")
        return d


def build_sample_table(slicers, image_size: int) -> VolumeSampleTable:
    """The table over one or more TrainingDataSlicer objects, in the order the train command numbers them (data0, data1, ...):
    sample i is the slice pair the PNG route's dataset holds at index i.  ``training_axes`` is read from each slicer's settings."""
    slicers = list(slicers)
    pairs = [volumes_as_ubyte(s) for s in slicers]
    axes = {utils.get_training_axis(s.settings) for s in slicers}
    if len(axes) != 1:
        raise ValueError("the slicers of one training run share their training_axes")
    store = _VolumeStore([p[0] for p in pairs], [p[1] for p in pairs])
    axis_enum, keep = axes.pop(), None
    if any(getattr(s, "ignore_label", None) is not None for s in slicers):
        check_ignore_label_occurs(slicers)
        for s in slicers:
            kept_slice_counts(s, axis_enum)
        keep = [s.labelled_slices for s in slicers]
    table = VolumeSampleTable(store, sample_order(store.shapes, axis_enum, keep=keep), image_size)
    table.ignore_label = utils.IGNORE_INDEX if keep is not None else None
    return table


# ---- the cut, in NumPy -----------------------------------------------------------------------------------------------------------
def _pad_map(n_out: int, offset: int, n: int, border: int) -> np.ndarray:
    """Padded-slice index of every output index: np.pad's "reflect" (reflect-101, continued periodically) or "edge"."""
    i = np.arange(n_out, dtype=np.int64) - offset
    if border == BORDER_EDGE or n == 1:
        return np.clip(i, 0, n - 1)
    period = 2 * (n - 1)
    i = np.mod(i, period)
    return np.where(i >= n, period - i, i)


def _cut_one(data: np.ndarray, labels: np.ndarray, d, size: int):
    h, w, nh, nw = int(d["h"]), int(d["w"]), int(d["nh"]), int(d["nw"])
    rs, cs = int(d["row_stride"]), int(d["col_stride"])
    grid = np.arange(h, dtype=np.int64)[:, None] * rs + np.arange(w, dtype=np.int64)[None, :] * cs
    img, msk = data[int(d["img_off"]) + grid], labels[int(d["msk_off"]) + grid]
    ry, rx = _pad_map(size, int(d["top"]), nh, int(d["border"])), _pad_map(size, int(d["left"]), nw, int(d["border"]))
    if (nh, nw) == (h, w):
        return img[np.ix_(ry, rx)], msk[np.ix_(ry, rx)]
    sy, sx = np.float32(np.float32(h) / np.float32(nh)), np.float32(np.float32(w) / np.float32(nw))
    # mask: cv2.resize INTER_NEAREST, floor(dst * scale) in fp32
    ny = np.minimum((ry.astype(np.float32) * sy).astype(np.int64), h - 1)
    nx = np.minimum((rx.astype(np.float32) * sx).astype(np.int64), w - 1)
    # image: INTER_LINEAR, source coordinate (dst + 0.5) * scale - 0.5 clipped to the slice; fp32 throughout, round half to even
    fy = np.clip((ry.astype(np.float32) + np.float32(0.5)) * sy - np.float32(0.5), np.float32(0), np.float32(h - 1))
    fx = np.clip((rx.astype(np.float32) + np.float32(0.5)) * sx - np.float32(0.5), np.float32(0), np.float32(w - 1))
    y0, x0 = np.floor(fy), np.floor(fx)
    wy, wx = (fy - y0)[:, None], (fx - x0)[None, :]
    y0, x0 = y0.astype(np.int64), x0.astype(np.int64)
    y1, x1 = np.minimum(y0 + 1, h - 1), np.minimum(x0 + 1, w - 1)      # beyond the last sample the weight is exactly 0
    f = img.astype(np.float32)
    one = np.float32(1)
    top = f[np.ix_(y0, x0)] * (one - wx) + f[np.ix_(y0, x1)] * wx
    bot = f[np.ix_(y1, x0)] * (one - wx) + f[np.ix_(y1, x1)] * wx
    out = top * (one - wy) + bot * wy
    return np.clip(np.rint(out), 0, 255).astype(np.uint8), msk[np.ix_(ny, nx)]


def cut_numpy(data: np.ndarray, labels: np.ndarray, descriptors: np.ndarray, size: int):
    """(images, masks), both (n, size, size) uint8: what vs_slices_cut_u8 writes for the same buffers and descriptors."""
    n = len(descriptors)
    images, masks = np.empty((n, size, size), np.uint8), np.empty((n, size, size), np.uint8)
    for j in range(n):
        images[j], masks[j] = _cut_one(data, labels, descriptors[j], size)
    return images, masks


def cut_device(data: torch.Tensor, labels: torch.Tensor, table_dev: torch.Tensor, size: int):
    """The same from device buffers through csrc/slice_feed.hip; table_dev: (n, 64) uint8 rows of vs_slice_cut on the device."""
    from .. import _lib
    n = table_dev.shape[0]
    images = torch.empty((n, size, size), dtype=torch.uint8, device=data.device)
    masks = torch.empty((n, size, size), dtype=torch.uint8, device=data.device)
    _lib.check(_lib.lib.vs_slices_cut_u8(_lib.ptr(data), data.numel(), _lib.ptr(labels), labels.numel(), _lib.ptr(table_dev), n, size,
                                         _lib.ptr(images), _lib.ptr(masks), _lib.stream_ptr()))
    return images, masks


class VolumeSliceLoader:
    """ResidentSliceLoader's contract over a VolumeSampleTable: the same ShardedBatchSampler decides the batches (`batch_sampler`,
    `set_epoch`), it yields (images (b, 1, s, s) uint8, masks (b, s, s) uint8) on the device - what `prepare_training_batch` takes
    for device-side augmentation / normalisation - or None for an empty validation share, and it makes the reference's label-range
    check once per loader.  What is resident is the volumes (shared by every loader over subsets of one table) and 64 bytes per
    sample; a batch is one launch of the cut kernel (NumPy on a CPU device)."""

    def __init__(self, table: VolumeSampleTable, batch_sampler, device):
        self.table, self.batch_sampler, self.device = table, batch_sampler, torch.device(device)
        self.num_labels = None      # set by the trainer: the label-range check of the reference's F.one_hot (see __iter__)
        self.size = table.image_size
        if self.device.type == "cuda":
            if self.size % 4:
                raise ValueError("VolumeSliceLoader: image_size must be a multiple of 4 on the GPU")
            self.data, self.labels = table.store.on(self.device)
            rows = np.ascontiguousarray(table.descriptors).view(np.uint8).reshape(len(table), CUT_DTYPE.itemsize)
            self.rows = torch.from_numpy(rows.copy()).to(self.device)
        self.max_label = self._max_label()

    def _cut(self, idx):
        if self.device.type == "cuda":
            i = torch.as_tensor(idx, dtype=torch.int64, device=self.device)
            return cut_device(self.data, self.labels, self.rows.index_select(0, i), self.size)
        images, masks = cut_numpy(self.table.store.data, self.table.store.labels, self.table.descriptors[np.asarray(idx, dtype=np.int64)],
                                  self.size)
        return torch.from_numpy(images), torch.from_numpy(masks)

    def _max_label(self) -> int:
        """Largest label among the FITTED masks of this subset - ResidentSliceLoader's number, so both feeds raise (or do not) on
        the same data: nearest-neighbour down-scaling can drop the one pixel that holds a slice's largest label, so the maximum
        over the source slices could differ.  A few launches per loader, a small chunk at a time."""
        best = -1
        for lo in range(0, len(self.table), _SCAN_CHUNK):
            masks = self._cut(list(range(lo, min(lo + _SCAN_CHUNK, len(self.table)))))[1]
            best = max(best, utils.max_real_label(masks, self.table.ignore_label))
        return best

    def __len__(self):
        return len(self.batch_sampler)

    def __iter__(self):
        if self.num_labels is not None and self.max_label >= self.num_labels:
            # the text of torch.nn.functional.one_hot, which the reference's prepare_training_batch raises on the first such batch
            raise RuntimeError("Class values must be smaller than num_classes.")
        for idx in self.batch_sampler:
            if not idx:
                yield None
                continue
            images, masks = self._cut(idx)
            yield images.unsqueeze(1), masks


def volume_feed_applies(settings) -> bool:
    """Whether batches are augmented on the device (a GPU, image_size a multiple of 8, no host augmentation asked for): the
    condition under which get_2d_training_dataloaders turns its resident feed on."""
    mode = getattr(settings, "augment", None) or ("device" if torch.cuda.is_available() and settings.image_size % 8 == 0 else "host")
    return mode == "device" and torch.cuda.is_available()


def _fits_device_memory(table: VolumeSampleTable, device: torch.device) -> bool:
    """This rank's verdict: the volumes and the table within a quarter of the free device memory (host memory is not rationed)."""
    if device.type != "cuda":
        return True
    free, _total = torch.cuda.mem_get_info(device)
    return table.nbytes <= free // 4


def _all_ranks_agree(fits: bool, world: int) -> bool:
    """One all-reduced minimum of the rank-local verdict: the volume feed is used by every rank or by none."""
    if world <= 1:
        return fits
    import torch.distributed as dist
    dev = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend() == "nccl" else torch.device("cpu")
    verdict = torch.tensor([1 if fits else 0], dtype=torch.int32, device=dev)
    dist.all_reduce(verdict, op=dist.ReduceOp.MIN)
    return bool(int(verdict.item()))


def get_volume_training_loaders(slicers, settings, rank: int = 0, world: int = 1, device=None):
    """(training loader, validation loader) of get_2d_training_dataloaders - the same shared split seed, 80/20 cut and
    samplers - fed from the volumes.  None when the volumes do not fit a quarter of the free device memory on SOME rank (the
    caller then takes the PNG route on every rank)."""
    batch_size = utils.get_batch_size(settings)
    table = build_sample_table(slicers, settings.image_size)
    n = len(table)
    seed = shared_seed(rank, world)
    indices = torch.randperm(n, generator=torch.Generator().manual_seed(seed)).tolist()
    cut = int(n * settings.training_set_proportion)
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
    device = torch.device(device)
    if not _all_ranks_agree(_fits_device_memory(table, device), world):
        logging.info(f"Training volumes of {table.nbytes / 2**30:.1f} GiB do not fit the volume feed's share (a quarter) of the free "
                     f"device memory on every rank: slicing to PNG files instead.")
        return None
    ts = ShardedBatchSampler(cut, batch_size, rank, world, shuffle=True, drop_last=True, seed=seed + 1)
    vs = ShardedBatchSampler(n - cut, batch_size, rank, world, shuffle=False, drop_last=False)
    return VolumeSliceLoader(table.subset(indices[:cut]), ts, device), VolumeSliceLoader(table.subset(indices[cut:]), vs, device)
