"""Smoothed-energy guidance (SEG; Hong, "Smoothed Energy Guidance: Guiding Diffusion Models with Reduced Energy Curvature of
Attention", NeurIPS 2024): host-side rules.

In the selected self-attention layers the queries of the perturbed batch rows are blurred over the token grid by a separable
Gaussian before a plain attention; the guidance then is PAG's, eps + s (c - p).  DESIGN.md section 7 states the contract.  This
module holds what needs no GPU: the kernel length per axis, the taps, the grid a layer runs on and the argument checks.  Layer
selection is `pag.select` (same expressions, same boundary rule)."""
from __future__ import annotations

import math
from typing import List, Tuple

from . import pag
from .lib import MACROS

DEFAULT_SEG_SCALE = 3.0
DEFAULT_SEG_BLUR_SIGMA = 100.0
MEAN_ABOVE = 9999.0            # a sigma beyond this (inf included) replaces the blur by the image's mean query
MAX_EXTENT = MACROS["IIR_SEG_MAX_EXTENT"]      # tokens per grid axis the blur launch takes (a 2048^2 image at level 1)


def check_sigma(seg_blur_sigma) -> float:
    if isinstance(seg_blur_sigma, bool) or not isinstance(seg_blur_sigma, (int, float)):
        raise ValueError(f"seg_blur_sigma must be a number > 0 (math.inf = the mean query), got {seg_blur_sigma!r}")
    s = float(seg_blur_sigma)
    if math.isnan(s) or s <= 0.0:
        raise ValueError(f"seg_blur_sigma must be > 0 (math.inf = the mean query), got {seg_blur_sigma!r}")
    return s


def check_scale(seg_scale) -> float:
    try:
        s = float(seg_scale)
    except (TypeError, ValueError):
        raise ValueError(f"seg_scale must be a finite number >= 0 (0 = off), got {seg_scale!r}") from None
    if not math.isfinite(s) or s < 0.0:
        raise ValueError(f"seg_scale must be a finite number >= 0 (0 = off), got {seg_scale!r}")
    return s


def is_mean(sigma: float) -> bool:
    return float(sigma) > MEAN_ABOVE


def kernel_length(sigma: float, n: int) -> int:
    """Taps along an axis of `n` tokens: k0 = ceil(6 sigma) rounded up to odd, capped at n + 1 (n even) or n (n odd), so that
    the half width k // 2 <= n - 1 and the reflect border is defined; n = 1 gives 1 (the axis is left alone)."""
    n = int(n)
    if n == 1:
        return 1
    cap = n + 1 if n % 2 == 0 else n
    if 6.0 * float(sigma) >= cap:                # (also keeps ceil away from huge or infinite sigma)
        return cap
    c = math.ceil(6.0 * float(sigma))
    return min(c + 1 - c % 2, cap)


def weights(sigma: float, n: int) -> List[float]:
    """Normalised Gaussian taps w_i ~ exp(-(x_i / sigma)^2 / 2), x_i = i - (k - 1) / 2, in fp64."""
    k = kernel_length(sigma, n)
    w = [math.exp(-0.5 * ((i - (k - 1) / 2.0) / float(sigma)) ** 2) for i in range(k)]
    tot = math.fsum(w)
    return [v / tot for v in w]


def level_grids(cfg, H: int, W: int) -> List[Tuple[int, int]]:
    """(h, w) of the token grid at each resolution level of the UNet for an H x W latent."""
    out = []
    for _ in cfg.block_out_channels:
        out.append((H, W))
        H, W = (H + 1) // 2, (W + 1) // 2
    return out


def path_level(cfg, path: str) -> int:
    """Resolution level of the `attn1` module `path` (`pag.attn1_paths` names)."""
    nb = len(cfg.block_out_channels)
    head, idx = path.split(".")[:2]
    if head == "mid_block":
        return nb - 1
    return int(idx) if head == "down_blocks" else nb - 1 - int(idx)


def check_grids(cfg, paths, H: int, W: int) -> None:
    """The blur launch takes grids up to MAX_EXTENT tokens per axis: a larger selected layer is refused here, before capture."""
    grids = level_grids(cfg, H, W)
    for p in paths:
        h, w = grids[path_level(cfg, p)]
        if h > MAX_EXTENT or w > MAX_EXTENT:
            raise ValueError(f"smoothed-energy guidance: {p} runs on a {h} x {w} token grid, the query blur takes at most "
                             f"{MAX_EXTENT} x {MAX_EXTENT}; select deeper layers (seg_applied_layers) or a smaller image")


def check_engine(net) -> None:
    """SEG needs the fp16 self-attention path, as PAG does: a UNet built with fp8 linears is refused."""
    if getattr(net, "fp8_linear", False):
        raise ValueError("enable_seg: this UNet was built with fp8 linears (fp8_linear=True); smoothed-energy guidance "
                         "runs on the fp16 engine only")


def select(layers, cfg) -> List[str]:
    return pag.select(layers, pag.attn1_paths(cfg), what="seg_applied_layers")
