"""The argument checks the device wrappers share (native_iou, native_track, native_aug, native_gtdb, native_eval).
Every check raises ValueError and reads nothing from the device; the wrappers run them before ``same_device``, so a
bad argument is reported whatever device the tensors are on.
"""
import math

import numpy as np
import torch


def _got(t):
    return (t.dtype, tuple(t.shape)) if torch.is_tensor(t) else type(t)


def _dt(dtype):
    return str(dtype).replace("torch.", "")


def strided_rows(t, name, min_cols, rows="n"):
    """fp32 [n, >= min_cols] with unit column stride (a view with a row stride will do) -> (n, the row stride)"""
    if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] < min_cols \
            or (t.shape[0] > 0 and t.stride(1) != 1) or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        raise ValueError(f"{name} must be an fp32 [{rows}, >= {min_cols}] tensor with unit column stride, got {_got(t)}")
    n = int(t.shape[0])
    return n, int(t.stride(0)) if n > 1 else int(t.shape[1])


def rows(t, name, widths=None, dtype=torch.float32):
    """a contiguous [n, c] tensor of the dtype with c in ``widths`` (None: [n]) -> t"""
    if not torch.is_tensor(t) or t.dtype != dtype or t.dim() != (1 if widths is None else 2) \
            or (widths is not None and t.shape[1] not in widths):
        want = "[n] tensor" if widths is None else f"[n, c] tensor with c in {list(widths)}"
        raise ValueError(f"{name} must be a {_dt(dtype)} {want}, got {_got(t)}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return t


def tensor(t, name, dtype, shape):
    """a contiguous tensor of the dtype and shape (None in ``shape``: any extent) -> t"""
    if (not torch.is_tensor(t) or t.dtype != dtype or t.dim() != len(shape) or not t.is_contiguous()
            or any(w is not None and int(g) != w for g, w in zip(t.shape, shape))):
        want = "[" + ", ".join("n" if w is None else str(w) for w in shape) + "]"
        raise ValueError(f"{name} must be a contiguous {_dt(dtype)} {want} tensor, got {_got(t)}")
    return t


def count_word(t, name="count"):
    """None or the device count of the valid rows: one int32 -> t"""
    if t is not None and (not torch.is_tensor(t) or t.dtype != torch.int32 or t.numel() != 1):
        raise ValueError(f"{name} must be one int32 on the device (a tensor of one element) or None, got {_got(t)}")
    return t


def same_device(dev, what, **tensors):
    """``dev`` is a HIP device and every tensor given (None entries pass) lives on it; ``what`` names the caller"""
    if dev.type != "cuda":
        raise ValueError(f"{what} on a HIP device (no CPU fallback)")
    for name, t in tensors.items():
        if t is not None and t.device != dev:
            raise ValueError(f"{name} is on {t.device}, expected {dev}")


def nonneg(v, name):
    v = float(v)
    if not math.isfinite(v) or v < 0:
        raise ValueError(f"{name} must be finite and not negative, got {v}")
    return v


def positive(v, name):
    v = float(v)
    if not math.isfinite(v) or v <= 0:
        raise ValueError(f"{name} must be finite and positive, got {v}")
    return v


def pose_arguments(pose):
    """A 4 x 4 (or 3 x 4) rigid pose, host array or tensor -> (12 floats row-major [R|t], pose_yaw):
    ``pose_yaw = atan2(R10, R00)`` in float64, rounded once to float32."""
    m = np.asarray(pose.detach().cpu().numpy() if torch.is_tensor(pose) else pose, dtype=np.float64)
    if m.shape not in ((4, 4), (3, 4)) or not np.isfinite(m).all():
        raise ValueError(f"pose must be a finite 4 x 4 (or 3 x 4) matrix, got shape {m.shape}")
    return [float(v) for v in m[:3].reshape(-1)], float(np.float32(math.atan2(m[1, 0], m[0, 0])))
