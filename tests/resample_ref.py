"""fp64 restatement of the resampling contract (DESIGN.md section 7 "Resampling"), written from the definition and not from
the product's table code (instantir_amd/resample.py), for the CPU and GPU resample tests.

An axis with input size n_in, output size n_out: scale = n_in / n_out, fs = max(scale, 1); output i has centre
c = (i + 0.5) * scale, taps x in [int(c - S fs + 0.5), int(c + S fs + 0.5)) clipped to [0, n_in), weights
f((x + 0.5 - c) / fs) normalised to sum 1; f = triangle (S = 1), Keys cubic a = -0.5 (S = 2), Lanczos-3 (S = 3).
Horizontal pass first, then vertical; an axis that keeps its size is skipped.  Quantised mode ends every pass in
clip(floor(v + 0.5), 0, 255); float mode rounds nowhere.

`resize(..., fp32=True)` runs the same operation order as the kernel in fp32: weights rounded to fp32, taps summed in
index order from 0 with a fused multiply-add (formed as an fp64 product-sum rounded to fp32: the product of two fp32
values is exact in fp64), quantisation and the clamp / affine tail in fp32."""
import math

import numpy as np

FILTERS = ("bilinear", "bicubic", "lanczos")
S = {"bilinear": 1.0, "bicubic": 2.0, "lanczos": 3.0}
U = 2.0 ** -24

# (H, W) -> (h, w) of the float / quantised GPU cases (tests/test_resample_gpu.py) and of the CPU rehearsal of their inputs
GPU_GEOMETRIES = [((37, 53), (64, 40)), ((96, 64), (37, 53)), ((1, 1), (8, 8)), ((5, 7), (1, 1)), ((3, 200), (200, 3)),
                  ((257, 131), (129, 67)), ((1024, 768), (256, 192))]
# in (H, W) -> out (H, W) of the comparisons with PIL
PIL_GEOMETRIES = [((37, 53), (64, 96)), ((96, 64), (37, 53)), ((200, 300), (56, 56)), ((40, 24), (163, 99)), ((61, 47), (224, 224))]


def f_of(name, x):
    x = abs(x)
    if name == "bilinear":
        return 1.0 - x if x < 1.0 else 0.0
    if name == "bicubic":
        a = -0.5
        if x < 1.0:
            return (a + 2.0) * x ** 3 - (a + 3.0) * x ** 2 + 1.0
        if x < 2.0:
            return a * x ** 3 - 5.0 * a * x ** 2 + 8.0 * a * x - 4.0 * a
        return 0.0
    if name == "lanczos":
        if x >= 3.0:
            return 0.0
        if x == 0.0:
            return 1.0
        return math.sin(math.pi * x) / (math.pi * x) * math.sin(math.pi * x / 3.0) / (math.pi * x / 3.0)
    raise ValueError(name)


def taps(n_in, n_out, name):
    """[(first tap, fp64 weights)] per output sample."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    rows = []
    for i in range(n_out):
        c = (i + 0.5) * scale
        lo = max(int(c - S[name] * fs + 0.5), 0)
        hi = min(int(c + S[name] * fs + 0.5), n_in)
        w = np.array([f_of(name, (x + 0.5 - c) / fs) for x in range(lo, hi)], dtype=np.float64)
        rows.append((lo, w / w.sum()))
    return rows


def abs_row_sum(n_in, n_out, name):
    """(L, taps): the largest row sum of |w| and the largest tap count of an axis (1, 1 for an axis that keeps its size)."""
    if n_in == n_out:
        return 1.0, 1
    rows = taps(n_in, n_out, name)
    return max(np.abs(w).sum() for _, w in rows), max(len(w) for _, w in rows)


def float_bound(in_hw, out_hw, name, max_abs):
    """Bound of |kernel - fp64 restatement| in float mode.  One pass sums n taps with fmaf from 0: n roundings, each at most
    2^-24 of a partial sum bounded by L * max|x| (L = the largest row sum of |w|); the fp32 weights differ from the fp64
    ones by 2^-24 relative, another 2^-24 * L * max|x|; one more unit covers the second-order terms:
        e_pass = (taps + 2) * 2^-24 * L * max|x|.
    Two passes compose: the vertical pass sees an input off by e_h and bounded by L_h * max|x| + e_h, so
        e = L_v * e_h + (taps_v + 2) * 2^-24 * L_v * (L_h * max|x| + e_h)."""
    (H, W), (h, w) = in_hw, out_hw
    Lh, th = abs_row_sum(W, w, name)
    Lv, tv = abs_row_sum(H, h, name)
    eh = (th + 2) * U * Lh * max_abs if W != w else 0.0
    mid = Lh * max_abs + eh
    ev = (tv + 2) * U * Lv * mid if H != h else 0.0
    return Lv * eh + ev


def _fma32(w, s, acc):
    return (np.float64(w) * s.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)


def _pass(x, n_out, name, axis, quantize, fp32):
    """x (..., H, W) -> the axis (-1: horizontal, -2: vertical) resampled to n_out."""
    x = np.moveaxis(x, axis, -1)
    out = np.empty(x.shape[:-1] + (n_out,), dtype=np.float32 if fp32 else np.float64)
    for i, (lo, w) in enumerate(taps(x.shape[-1], n_out, name)):
        if fp32:
            acc = np.zeros(x.shape[:-1], dtype=np.float32)
            for k, wk in enumerate(w.astype(np.float32)):
                acc = _fma32(wk, x[..., lo + k], acc)
        else:
            acc = np.zeros(x.shape[:-1], dtype=np.float64)
            for k, wk in enumerate(w):
                acc = acc + wk * x[..., lo + k]
        out[..., i] = acc
    if quantize:
        half = np.float32(0.5) if fp32 else 0.5
        out = np.clip(np.floor(out + half), 0, 255)
    return np.moveaxis(out, -1, axis)


def resize(x, size, name, quantize=False, fp32=False, window=None, clamp=None, scale=None, bias=None):
    """x (N, C, H, W) -> (N, C, h, w) [its window (y0, x0, h, w)], then clamp (lo, hi), then v * scale[c] + bias[c]."""
    x = np.asarray(x, dtype=np.float32 if fp32 else np.float64)
    h, w = size
    same = x.shape[-2:] == (h, w)
    if x.shape[-1] != w:
        x = _pass(x, w, name, -1, quantize, fp32)
    if x.shape[-2] != h:
        x = _pass(x, h, name, -2, quantize, fp32)
    if same and quantize:
        x = np.clip(np.floor(x + (np.float32(0.5) if fp32 else 0.5)), 0, 255)
    if window is not None:
        y0, x0, hh, ww = window
        x = x[:, :, y0:y0 + hh, x0:x0 + ww]
    dt = np.float32 if fp32 else np.float64
    if clamp is not None:
        x = np.clip(x, dt(clamp[0]), dt(clamp[1]))
    if scale is not None:
        x = x * np.asarray(scale, dtype=np.float32).astype(dt).reshape(1, -1, 1, 1)
    if bias is not None:
        x = x + np.asarray(bias, dtype=np.float32).astype(dt).reshape(1, -1, 1, 1)
    return x


def noise_u8(seed, N, H, W, C):
    """Full-range seeded uint8 noise, interleaved (N, H, W, C)."""
    return np.random.default_rng(seed).integers(0, 256, (N, H, W, C), dtype=np.uint8)


def planar(u8):
    return np.ascontiguousarray(np.transpose(u8, (0, 3, 1, 2)))


def pil_resize(u8_hwc, size, name):
    """PIL's own resize of one uint8 (H, W, C) image to size = (h, w)."""
    from PIL import Image
    flt = {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}[name]
    im = Image.fromarray(u8_hwc[:, :, 0] if u8_hwc.shape[2] == 1 else u8_hwc)
    out = np.asarray(im.resize((size[1], size[0]), flt))
    return out[:, :, None] if out.ndim == 2 else out


def lsb_report(a, b):
    """(largest |a - b|, fraction of samples that differ)."""
    d = np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))
    return float(d.max()), float((d != 0).mean())
