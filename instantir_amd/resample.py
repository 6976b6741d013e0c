"""Device-side image resampling with PIL's filter definitions (DESIGN.md section 7 "Resampling"): the host side of
`iir_resample_pass`.

`Image.resize` is a separable, antialiased resampler.  For an axis with input size `n_in`, output size `n_out`,
scale = n_in / n_out and fs = max(scale, 1), output sample i has centre c = (i + 0.5) * scale, taps the input indices in
[int(c - S fs + 0.5), int(c + S fs + 0.5)) clipped to the image, and weights f((x + 0.5 - c) / fs) normalised to sum 1, with
f the triangle (S = 1), the Keys cubic with a = -0.5 (S = 2) or Lanczos-3 (S = 3).  `coefficients` builds these tables in
PIL's `precompute_coeffs` layout (first tap and tap count per output sample, `ksize` zero-padded weights per output sample)
in fp64, rounded to fp32; `device_tables` caches them on the device per (n_in, n_out, filter).  The difference from PIL
is the weights' format: fp32 here, 22-bit fixed point there, hence at most 1 LSB on 8-bit images.

`ops.resample` launches the passes on a device tensor; `resize_images` is the front door for PIL / numpy / tensor input
(one uint8 upload for 8-bit images: 3 bytes per pixel on the bus).
"""
from __future__ import annotations

import math

import numpy as np
import torch

from .lib import MACROS

FILTERS = ("bilinear", "bicubic", "lanczos")
SUPPORT = {"bilinear": 1.0, "bicubic": 2.0, "lanczos": 3.0}
MAX_SIDE = MACROS["IIR_RESAMPLE_MAX_SIDE"]
MAX_PLANES = 65535          # N * C of one launch


def _bilinear(x):
    x = np.abs(x)
    return np.where(x < 1.0, 1.0 - x, 0.0)


def _bicubic(x, a=-0.5):
    x = np.abs(x)
    near = ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0
    far = (((x - 5.0) * x + 8.0) * x - 4.0) * a
    return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))


def _lanczos(x):
    inside = np.abs(x) < 3.0
    return np.where(inside, np.sinc(x) * np.sinc(x / 3.0), 0.0)          # np.sinc(x) = sin(pi x) / (pi x), 1 at 0


_KERNELS = {"bilinear": _bilinear, "bicubic": _bicubic, "lanczos": _lanczos}


def _check_filter(filter, who="resample"):
    if filter not in FILTERS:
        raise ValueError(f"{who}: filter must be one of {FILTERS}, got {filter!r}")


def coefficients(in_size, out_size, filter):
    """The tables of one axis: (bounds int32 (out_size, 2) = {first tap, tap count}, weights fp32 (out_size, ksize))."""
    _check_filter(filter, "coefficients")
    in_size, out_size = int(in_size), int(out_size)
    if in_size <= 0 or out_size <= 0:
        raise ValueError(f"coefficients: sizes must be positive, got {in_size} -> {out_size}")
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = SUPPORT[filter] * fs
    ksize = int(math.ceil(support)) * 2 + 1
    centre = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    first = np.clip(np.trunc(centre - support + 0.5), 0, None).astype(np.int64)
    last = np.clip(np.trunc(centre + support + 0.5), None, in_size).astype(np.int64)
    count = last - first
    k = np.arange(ksize, dtype=np.int64)[None, :]
    w = _KERNELS[filter]((k + first[:, None] + 0.5 - centre[:, None]) / fs)
    w = np.where(k < count[:, None], w, 0.0)
    total = w.sum(axis=1, keepdims=True)
    w = np.where(total != 0.0, w / np.where(total != 0.0, total, 1.0), w)
    return np.stack([first, count], axis=1).astype(np.int32), w.astype(np.float32)


def identity_tables(size):
    """One tap of weight 1 per sample: a pass that only converts layout, cuts a window or applies the per-launch options."""
    idx = np.arange(int(size), dtype=np.int32)
    return np.stack([idx, np.ones_like(idx)], axis=1), np.ones((int(size), 1), dtype=np.float32)


_tables = {}
_vectors = {}


def device_tables(in_size, out_size, filter, device):
    """(bounds, weights, ksize) of one axis on `device`, built once per (in_size, out_size, filter); filter None: identity."""
    device = torch.device(device)
    key = (int(in_size), int(out_size), filter, device)
    if key not in _tables:
        b, w = identity_tables(in_size) if filter is None else coefficients(in_size, out_size, filter)
        _tables[key] = (torch.from_numpy(b).contiguous().to(device), torch.from_numpy(w).contiguous().to(device), int(w.shape[1]))
    return _tables[key]


def channel_vector(value, C, device, name):
    """`scale` / `bias` of a launch as fp32 (C,) on the device: None, a number, C numbers, or a tensor of C values."""
    if value is None:
        return None
    if torch.is_tensor(value):
        if value.numel() != C:
            raise ValueError(f"resample: {name} must hold one value per channel ({C}), got {value.numel()}")
        return value.to(device, torch.float32).reshape(C).contiguous()
    vals = (float(value),) * C if isinstance(value, (int, float)) else tuple(float(v) for v in value)
    if len(vals) != C:
        raise ValueError(f"resample: {name} must hold one value per channel ({C}), got {len(vals)}")
    key = (vals, torch.device(device))
    if key not in _vectors:
        _vectors[key] = torch.tensor(vals, dtype=torch.float32).to(device)
    return _vectors[key]


def check_size(size, what="size", multiple=None):
    """`size` as (H, W) ints; ValueError otherwise."""
    try:
        h, w = (int(v) for v in size)
        ok = len(tuple(size)) == 2 and all(float(v) == int(v) for v in size)
    except (TypeError, ValueError):
        ok = False
    if not ok or h <= 0 or w <= 0 or h > MAX_SIDE or w > MAX_SIDE:
        raise ValueError(f"{what} must be (H, W) with 1 <= H, W <= {MAX_SIDE}, got {size!r}")
    if multiple and (h % multiple or w % multiple):
        raise ValueError(f"{what} {(h, w)} must be a multiple of {multiple}")
    return h, w


def check_args(size, filter, quantize, window, clamp):
    """The geometry-free checks of `ops.resample`; returns (oh, ow), (y0, x0, h, w), clamp or None."""
    _check_filter(filter)
    oh, ow = check_size(size, "resample: size")
    if window is None:
        win = (0, 0, oh, ow)
    else:
        try:
            win = tuple(int(v) for v in window)
        except (TypeError, ValueError):
            win = ()
        if len(win) != 4:
            raise ValueError(f"resample: window must be (y0, x0, h, w), got {window!r}")
        y0, x0, h, w = win
        if y0 < 0 or x0 < 0 or h <= 0 or w <= 0 or y0 + h > oh or x0 + w > ow:
            raise ValueError(f"resample: window {win} does not lie inside the output {(oh, ow)}")
    if clamp is not None:
        try:
            lo, hi = (float(v) for v in clamp)
        except (TypeError, ValueError):
            raise ValueError(f"resample: clamp must be (lo, hi), got {clamp!r}")
        if not lo <= hi:
            raise ValueError(f"resample: clamp needs lo <= hi, got {clamp!r}")
        clamp = (lo, hi)
    if not isinstance(quantize, (bool, np.bool_)):
        raise ValueError(f"resample: quantize must be a bool, got {quantize!r}")
    return (oh, ow), win, clamp


def as_batch(images):
    """PIL image(s), numpy array(s) or a tensor as one batch: (array, "u8") with a uint8 (N, H, W, C) numpy array, or
    (tensor, "f32") with an fp32 (N, C, H, W) tensor.  8-bit inputs stay 8-bit: that is what gets uploaded."""
    if torch.is_tensor(images):
        t = images
        if t.dtype == torch.uint8:
            if t.dim() == 3:
                t = t.unsqueeze(0)
            if t.dim() != 4:
                raise ValueError(f"resize_images: a uint8 tensor must be (H, W, C) or (N, H, W, C), got {tuple(images.shape)}")
            return t, "u8"
        if t.dim() == 3:
            t = t.unsqueeze(0)
        if t.dim() != 4 or not t.is_floating_point():
            raise ValueError(f"resize_images: a float tensor must be (C, H, W) or (N, C, H, W), got {images.dtype} {tuple(images.shape)}")
        return t.to(torch.float32), "f32"
    items = list(images) if isinstance(images, (list, tuple)) else [images]
    if not items:
        raise ValueError("resize_images: no images")
    arrs = []
    for im in items:
        if hasattr(im, "convert"):
            im = im if im.mode in ("L", "RGB", "RGBA") else im.convert("RGB")
        a = np.asarray(im)
        if a.ndim == 2:
            a = a[:, :, None]
        arrs.append(a)
    if len({a.shape for a in arrs}) != 1 or len({a.dtype for a in arrs}) != 1:
        raise ValueError("resize_images: images of one batch must share one size and type")
    a = arrs[0] if (len(arrs) == 1 and arrs[0].ndim == 4 and not isinstance(images, (list, tuple))) else np.stack(arrs)
    if a.ndim != 4:
        raise ValueError(f"resize_images: images must be (H, W[, C]) each, got {arrs[0].shape}")
    if a.dtype == np.uint8:
        return np.ascontiguousarray(a), "u8"
    if a.dtype.kind != "f":
        raise ValueError(f"resize_images: arrays must be uint8 or floating point, got {a.dtype}")
    return torch.from_numpy(np.ascontiguousarray(a.astype(np.float32))).permute(0, 3, 1, 2), "f32"


def resize_images(images, size, filter="bilinear", device=None, quantize=None, window=None, clamp=None, scale=None, bias=None):
    """Resize PIL / numpy / tensor image(s) to `size` = (H, W) on `device`; fp32 (N, C, h, w) on the device comes back.
    8-bit inputs (PIL, uint8 arrays or tensors, (N, H, W, C)) are uploaded as they are and keep 0..255 units; `quantize`
    defaults to True for them (PIL's semantics for such an image) and to False for float input ((N, C, H, W), any range).
    `window`, `clamp`, `scale`, `bias`: as for `ops.resample`."""
    from . import ops
    batch, kind = as_batch(images)
    if quantize is None:
        quantize = kind == "u8"
    check_args(size, filter, bool(quantize), window, clamp)
    if device is None:
        device = batch.device if torch.is_tensor(batch) and batch.is_cuda else torch.device("cuda:0")
    src = (batch if torch.is_tensor(batch) else torch.from_numpy(batch)).to(device).contiguous()
    return ops.resample(src, size, filter, quantize=bool(quantize), window=window, clamp=clamp, scale=scale, bias=bias)
