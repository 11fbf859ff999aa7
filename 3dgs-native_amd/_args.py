"""Argument predicates and validators shared by the feature modules: what a caller's tensor, image, scalar or camera must be,
judged before the library or the GPU is touched.  Checks that belong to one feature only live in that feature's module."""
import math

import numpy as np
import torch


def is_dev(t, dtype):
    return isinstance(t, torch.Tensor) and t.dtype == dtype and t.is_cuda


def is_f32(x):
    """A torch tensor or numpy array of float32."""
    return x.dtype == (torch.float32 if isinstance(x, torch.Tensor) else np.float32)


def is_packed(t, n=None):
    """A contiguous float32 device tensor (of n elements); the caller words the refusal.  Adam asks this twenty times an iteration:
    one call deep."""
    return isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.is_cuda and t.is_contiguous() and (n is None or t.numel() == n)


def check_out(t, shape, name, dtype=torch.float32, dev=None):
    """A caller-owned output: a `dtype` device tensor (on `dev`) of this shape, contiguous and 16-byte aligned (include/gsr.h)."""
    if not (is_dev(t, dtype) and (dev is None or t.device == dev) and tuple(t.shape) == tuple(shape) and t.is_contiguous()
            and t.data_ptr() % 16 == 0):
        raise ValueError(f"{name} must be a contiguous, 16-byte aligned {str(dtype).replace('torch.', '')} device tensor of shape {tuple(shape)}"
                         + ("" if dev is None else f" on {dev}"))


def check_slot(t, n, name, contiguous=False):
    """An optional result slot: None, or n float32 on the device -- an element or a row of a larger tensor goes through as it is."""
    if t is not None and not (is_dev(t, torch.float32) and t.numel() == n and (not contiguous or t.is_contiguous())):
        raise ValueError(f"{name} must be a {'contiguous ' if contiguous else ''}{n}-element float32 device tensor")


def check_one_device(*xs):
    devs = {x.device for x in xs if isinstance(x, torch.Tensor) and x.is_cuda}
    if len(devs) > 1:
        raise ValueError(f"all tensors must live on one device (got {sorted(str(d) for d in devs)})")


def image_hw(x, name, hw=None, channels=None, squeeze=True, f32=False):
    """(H, W) of an image as given: shape (H, W) -- or (H, W, 1) with `squeeze` -- without `channels`, (H, W, channels) with;
    H, W >= 1, and equal to `hw` when the size is known.  `f32`: also a torch tensor or numpy array of float32."""
    if f32 and not isinstance(x, (torch.Tensor, np.ndarray)):
        raise ValueError(f"{name} must be a torch tensor or a numpy array, not {type(x).__name__}")
    given = tuple(np.shape(x))
    if channels is None:
        got = given[:2] if squeeze and len(given) == 3 and given[2] == 1 else given
    else:
        got = given[:2] if len(given) == 3 and given[2] == channels else None
    tail = () if channels is None else (channels,)
    if hw is not None:
        if got != tuple(hw):
            raise ValueError(f"{name} must have shape {tuple(hw) + tail} (the image's shape), not {given}")
    elif got is None or len(got) != 2 or got[0] < 1 or got[1] < 1:
        raise ValueError(f"{name} must have shape {'(H, W)' if channels is None else f'(H, W, {channels})'}, not {given}")
    if f32 and not is_f32(x):
        raise ValueError(f"{name} must be float32, not {x.dtype}")
    return got


def _number(x, name):
    try:
        return float(x)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a number, not {x!r}") from None


def finite(x, name):
    v = _number(x, name)
    if not math.isfinite(v):
        raise ValueError(f"{name} must be finite, not {x}")
    return v


def positive(x, name, allow_inf=False):
    v = _number(x, name)
    if not v > 0.0 or (math.isinf(v) and not allow_inf):
        raise ValueError(f"{name} must be positive{'' if allow_inf else ' and finite'}, not {x}")
    return v


def camera_params(camera, who):
    """(tan_fovx, tan_fovy, W, H) of a camera dict."""
    try:
        tx, ty, W, H = float(camera["tan_fovx"]), float(camera["tan_fovy"]), camera["width"], camera["height"]
    except (KeyError, TypeError, IndexError):
        raise ValueError(f"{who}: camera must be a dict with tan_fovx, tan_fovy, width and height") from None
    if not (math.isfinite(tx) and math.isfinite(ty) and tx > 0.0 and ty > 0.0):
        raise ValueError(f"{who}: tan_fovx and tan_fovy must be positive and finite, not {tx}, {ty}")
    if int(W) != W or int(H) != H or W < 1 or H < 1 or int(W) * int(H) > 1 << 28:
        raise ValueError(f"{who}: width and height must be integers >= 1 with width * height <= 2^28, not {W} x {H}")
    return tx, ty, int(W), int(H)
