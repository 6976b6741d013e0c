"""What the scoring modules (metrics, lpips, niqe) agree on before anything is uploaded: which image forms they accept, the
layout the kernels read, the crop option and the device default.  No GPU is needed to import or call this module, so every
host-side refusal fires before an upload.  The device side of the same agreement is csrc/image_common.h.
"""
from __future__ import annotations

import numpy as np
import torch


def _pil_array(im):
    if im.mode not in ("L", "RGB"):
        im = im.convert("RGB")
    a = np.array(im)
    return a[:, :, None] if a.ndim == 2 else a


def host_source(x, arg):
    """A PIL image or a list of them, a numpy array (H, W), (H, W, C) or (N, H, W, C), a uint8 tensor in those layouts or a float
    tensor (C, H, W) / (N, C, H, W) -> (host tensor in the kernels' layout: uint8 (N, H, W, C) or fp32 (N, C, H, W); whether the
    argument was one image)."""
    from PIL import Image
    if isinstance(x, Image.Image):
        return torch.from_numpy(np.ascontiguousarray(_pil_array(x)[None])), True
    if isinstance(x, (list, tuple)):
        if not x or not all(isinstance(im, Image.Image) for im in x):
            raise ValueError(f"{arg}: a list must hold PIL images (at least one)")
        arrs = [_pil_array(im) for im in x]
        if len({a.shape for a in arrs}) != 1:
            raise ValueError(f"{arg}: the images of a list must share a size and a mode, got {sorted({a.shape for a in arrs})}")
        return torch.from_numpy(np.stack(arrs)), False
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x))
        channels_last = True
    elif torch.is_tensor(x):
        channels_last = x.dtype == torch.uint8
    else:
        raise ValueError(f"{arg}: expected a PIL image, a list of PIL images, a numpy array or a tensor, got {type(x).__name__}")
    if x.dtype != torch.uint8 and not x.dtype.is_floating_point:
        raise ValueError(f"{arg}: expected uint8 or floating-point values, got {x.dtype}")
    single = x.dim() < 4
    if channels_last:                   # (H, W), (H, W, C), (N, H, W, C)
        if x.dim() == 2:
            x = x[None, :, :, None]
        elif x.dim() == 3:
            x = x[None]
    elif x.dim() == 3:                  # (C, H, W)
        x = x[None]
    if x.dim() != 4:
        raise ValueError(f"{arg}: expected an image or a batch of images, got shape {tuple(x.shape)}")
    if x.dtype != torch.uint8:
        x = x.float()
        if channels_last:
            x = x.permute(0, 3, 1, 2)
    return x, single


def dims(t):
    """(N, C, H, W) of a tensor in either kernel layout."""
    return tuple(t.shape[i] for i in (0, 3, 1, 2)) if t.dtype == torch.uint8 else tuple(t.shape)


def check_crop(who, crop_border):
    if isinstance(crop_border, bool) or not isinstance(crop_border, int) or crop_border < 0:
        raise ValueError(f"{who}: crop_border must be an integer >= 0, got {crop_border!r}")


def scoring_device(device, who="instantir_amd.metrics"):
    """`device` as a torch.device; the current GPU when None, and an error where there is none."""
    if device is not None:
        return torch.device(device)
    if not torch.cuda.is_available():
        raise RuntimeError(f"{who} needs an MI355X: image scoring has no host path")
    return torch.device("cuda", torch.cuda.current_device())
