"""The ground the analyses of a finished label volume share (evaluation, surface_distance, components, measurements, meshes): the
shape as (Z, Y, X), where to work, whether the device has room, the volume as uint8 bytes, and a few rules of their reports.  It
imports none of them.

A volume is a host array or a device tensor of one to three dimensions.  ``prepare`` is the whole way in for the analyses that take
label bytes as they are; those that first map values to classes use the same pieces in their own order."""
from __future__ import annotations

import numpy as np


# ---- shapes, tensors, devices ------------------------------------------------------------------------------------------------------
def zyx(shape) -> tuple[int, int, int]:
    shape = tuple(int(s) for s in shape)
    if not 1 <= len(shape) <= 3 or any(s < 1 for s in shape):
        raise ValueError(f"expected a non-empty volume of one to three dimensions, got shape {shape}")
    return (1,) * (3 - len(shape)) + shape


def is_tensor(x) -> bool:
    return type(x).__module__.startswith("torch") and hasattr(x, "data_ptr")


def is_resident(x, device=None) -> bool:
    """a tensor on a GPU - on ``device``, where one is given"""
    return is_tensor(x) and x.is_cuda and (device is None or x.device == device)


def to_host(x) -> np.ndarray:
    return x.detach().cpu().numpy() if is_tensor(x) else np.asarray(x)


def aligned_u8(x, device):
    """the volume as flat, contiguous, 16-byte aligned uint8 device memory"""
    import torch

    x = (x if is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))).to(device).contiguous().reshape(-1)
    return x if x.data_ptr() % 16 == 0 else x.clone()


def pick_device(device, *arrays):
    """the GPU to work on: ``device`` where given, else that of the first resident tensor among ``arrays``, else the current GPU; None
    - the host route - for ``"cpu"`` or where there is no GPU"""
    import torch
    if device is None:
        src = next((a for a in arrays if is_resident(a)), None)
        device = src.device if src is not None else (torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None)
    device = None if device is None else torch.device(device)
    return device if device is not None and device.type == "cuda" else None


def require_memory(device, need: int, what: str) -> None:
    import torch
    free, _ = torch.cuda.mem_get_info(device)
    if need > free:
        raise ValueError(f"{what} needs {need} bytes of device memory but only {free} bytes are free on {device}")


# ---- uint8 bytes -------------------------------------------------------------------------------------------------------------------
def is_u8(x) -> bool:
    if is_tensor(x):
        import torch
        return x.dtype == torch.uint8
    return np.asarray(x).dtype == np.uint8


def strict_u8(vol):
    """the volume as uint8 - a host array or a device tensor as it came - after checking that every value fits.  For the analyses that
    read label VALUES (components, measurements, meshes): a value that does not fit has no byte to stand for it, so it raises."""
    if is_tensor(vol):
        import torch
        if vol.dtype == torch.uint8:
            return vol
        if vol.dtype == torch.bool:
            return vol.to(torch.uint8)
        if vol.dtype.is_floating_point or vol.dtype.is_complex:
            raise TypeError(f"expected an integer label volume, got {vol.dtype}")
        lo, hi = int(vol.min()), int(vol.max())
        if lo < 0 or hi > 255:
            raise ValueError(f"label values {lo}..{hi} do not fit uint8")
        return vol.to(torch.uint8)
    a = np.asarray(vol)
    if a.dtype == np.uint8:
        return a
    if a.dtype == np.bool_:
        return a.astype(np.uint8)
    if not np.issubdtype(a.dtype, np.integer):
        raise TypeError(f"expected an integer label volume, got {a.dtype}")
    if a.size and (int(a.min()) < 0 or int(a.max()) > 255):
        raise ValueError(f"label values {int(a.min())}..{int(a.max())} do not fit uint8")
    return a.astype(np.uint8)


def lenient_u8(pred):
    """predicted class indices as uint8 - as they came where they are uint8, else converted on the host; whatever does not fit becomes
    255, which no class count reaches.  For the scores (evaluation, surface_distance): there a misfit is a voxel to count as invalid
    or to leave out of every class, not a reason to stop."""
    if is_u8(pred):
        return pred
    pred = to_host(pred)
    if pred.dtype == np.bool_:
        return pred.astype(np.uint8)
    if not np.issubdtype(pred.dtype, np.integer):
        raise TypeError(f"predictions must be an integer label volume, got {pred.dtype}")
    out = pred.astype(np.uint8)
    out[(pred < 0) | (pred > 254)] = 255
    return out


def prepare(vol, device, need, what: str):
    """(shape, zyx, device or None, the label bytes): a host (Z, Y, X) array where the device is None, else flat aligned device memory.
    ``need(zyx, resident)`` is the device memory in bytes the caller is about to take, the upload included unless the volume is
    ``resident``; it is checked against the free memory before the upload, under the name "the ``what`` of a ``shape`` volume"."""
    shape = tuple(vol.shape)
    extents = zyx(shape)
    device = pick_device(device, vol)
    v = strict_u8(vol)
    if device is None:
        return shape, extents, None, np.ascontiguousarray(to_host(v)).reshape(extents)
    bytes_needed = need(extents, is_resident(v))
    if bytes_needed:
        require_memory(device, bytes_needed, f"the {what} of a {shape} volume")
    return shape, extents, device, aligned_u8(v, device)


# ---- rules of the reports ----------------------------------------------------------------------------------------------------------
def touch_mask(zyx) -> np.ndarray:
    """(Z, Y, X) bool: the voxels with a coordinate equal to 0 or to extent - 1 on an axis longer than 1"""
    face = np.zeros(zyx, dtype=bool)
    for axis, extent in enumerate(zyx):
        if extent > 1:
            s = [slice(None)] * 3
            s[axis] = [0, extent - 1]
            face[tuple(s)] = True
    return face


def voxel_size(voxel_size) -> tuple[float, float, float]:
    """a scalar or [sz, sy, sx], each positive"""
    size = np.asarray(voxel_size, dtype=np.float64).reshape(-1)
    if size.size == 1:
        size = np.repeat(size, 3)
    if size.size != 3 or not np.all(np.isfinite(size)) or not np.all(size > 0):
        raise ValueError(f"voxel size {voxel_size!r}: it is one positive number or three, [sz, sy, sx]")
    return float(size[0]), float(size[1]), float(size[2])


MAX_WEIGHT = 64               # the largest integer weight of an axis (csrc/surface.hip: vs_edt_squared_scaled)
UNIT_WEIGHTS = (1, 1, 1)


def voxel_grid(spacing) -> tuple[tuple[int, int, int], float]:
    """``(weights (wz, wy, wx), unit u)`` of ``voxel_spacing: [sz, sy, sx]``: positive integers with gcd 1, each at most 64, with ``s_i =
    w_i u``.  The weight of the smallest step is the first ``m`` in 1..64 for which every ``s_i / s_min * m`` lies within 1e-6 relative of
    an integer at most 64, and ``u = s_min / m``.  With ``q_i = w_i^2`` the squared distance between two voxels is the integer ``D = qz dz^2
    + qy dy^2 + qx dx^2`` and a physical distance is ``u sqrt(D)``.  Steps in no such ratio are refused."""
    try:
        size = np.asarray(spacing, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        size = np.zeros(0)
    if size.size != 3 or not np.all(np.isfinite(size)) or not np.all(size > 0):
        raise ValueError(f"voxel_spacing {spacing!r}: it is three finite positive numbers, [sz, sy, sx]")
    smallest = float(size.min())
    for m in range(1, MAX_WEIGHT + 1):
        scaled = size / smallest * m
        w = np.rint(scaled)
        if np.all(np.abs(scaled - w) <= 1e-6 * scaled) and np.all(w >= 1) and np.all(w <= MAX_WEIGHT):
            return (int(w[0]), int(w[1]), int(w[2])), smallest / m         # the first such m leaves no common factor
    raise ValueError(f"voxel_spacing {spacing!r}: the steps must be in a ratio of integers of at most {MAX_WEIGHT} for distances to stay exact "
                     f"integers - round the steps, for example to two significant digits")


def check_weights(weights, zyx) -> tuple[int, int, int]:
    """the integer weights of the axes as a tuple, after checking that every weighted squared distance of a ``zyx`` volume fits below
    2^32 - 1; an axis of length 1 contributes nothing"""
    w = tuple(int(x) for x in weights)
    if len(w) != 3 or any(not 1 <= x <= MAX_WEIGHT for x in w):
        raise ValueError(f"weights {weights!r}: three integers of 1..{MAX_WEIGHT}")
    most = sum(x * x * (e - 1) ** 2 for x, e in zip(w, zyx))
    if most >= 0xFFFFFFFF:
        raise ValueError(f"a volume of shape {tuple(zyx)} under the weights {w} can hold a squared distance of {most}: wz^2 (Z-1)^2 + wy^2 (Y-1)^2 + "
                         f"wx^2 (X-1)^2 must be below 2^32 - 1 = 4294967295")
    return w


def grid_of(spacing, zyx) -> tuple[tuple[int, int, int], float]:
    """``voxel_grid`` for a ``spacing=`` argument: None is the unit grid; the weights are checked against the volume"""
    if spacing is None:
        return UNIT_WEIGHTS, 1.0
    weights, unit = voxel_grid(spacing)
    return check_weights(weights, zyx), unit


def spacing_settings(settings, *scalar_keys):
    """the optional predict-settings key ``voxel_spacing`` as ``(spacing [sz, sy, sx] as floats, weights, unit)``, or None where the key is
    absent.  ``scalar_keys``: the per-analysis keys that hold ONE voxel size - setting one of them beside ``voxel_spacing`` is an error,
    for a scalar cannot override a grid."""
    spacing = getattr(settings, "voxel_spacing", None)
    if spacing is None:
        return None
    weights, unit = voxel_grid(spacing)
    for key in scalar_keys:
        if getattr(settings, key, None) is not None:
            raise ValueError(f"voxel_spacing and {key} are both set: {key} is one number and cannot override the grid of voxel_spacing - "
                             f"remove one of the two keys")
    return [float(s) for s in np.asarray(spacing, dtype=np.float64).reshape(-1)], weights, unit


def json_number(x):
    """a float for a JSON document: NaN is written as null, infinity as the string "inf" """
    x = float(x)
    return None if np.isnan(x) else "inf" if np.isinf(x) else x


def percentile_from_counts(values: np.ndarray, counts: np.ndarray, q: float) -> float:
    """NumPy's default (linear) percentile of the multiset that holds values[i] counts[i] times; values ascending"""
    total = int(counts.sum())
    cum = np.cumsum(counts)
    virtual = (total - 1) * (q / 100.0)
    lo = int(np.floor(virtual))
    hi = min(lo + 1, total - 1)
    t = virtual - lo
    a = float(values[np.searchsorted(cum, lo, side="right")])
    b = float(values[np.searchsorted(cum, hi, side="right")])
    return a + (b - a) * t if t < 0.5 else b - (b - a) * (1.0 - t)
