"""Synthetic degradation (DESIGN.md section 7 "Synthetic degradation"): the host side of `iir_filter2d_f32`,
`iir_add_gaussian_noise_f32` and `iir_jpeg_roundtrip_f32` -- blur-kernel builders, reproducible recipes and `degrade`, which
turns clean images into low-quality ones on the device.  It stands where the reference's `RealESRGANDegradation`
(utils/degradation_pipeline.py) stands, without basicsr or cv2; numpy only.

A `Recipe` is data: a list of `Stage`s (blur, resize, noise, JPEG, in that order), the final low-pass (sinc) filter that goes
with the resize to 1 / sf of the input size, which side of that resize the last stage's JPEG falls on, and whether the result
goes back to the input's size.  `sample_recipe` draws one from a preset as a pure function of (preset, seed, name).
"""
from __future__ import annotations

import dataclasses
import json
import math
import zlib
from typing import List, Optional

import numpy as np
import torch

from .lib import MACROS

KSIZE_MAX = MACROS["IIR_FILTER2D_MAX_KSIZE"]
KERNEL_SIZES = tuple(range(7, KSIZE_MAX + 1, 2))     # utils/degradation_pipeline.py:106
PRESETS = ("realesrgan", "bicubic")

# The ranges and probabilities of the reference's KERNEL_OPT / DEGRADE_OPT (utils/degradation_pipeline.py:20-64), one entry per
# stage of the second-order chain.  kernel_prob follows KERNEL_KINDS.
KERNEL_KINDS = ("iso", "aniso", "generalized_iso", "generalized_aniso", "plateau_iso", "plateau_aniso")
REALESRGAN = {
    "kernel_prob": (0.45, 0.25, 0.12, 0.03, 0.12, 0.03),
    "sinc_prob": (0.1, 0.1),
    "blur_sigma": ((0.2, 3.0), (0.2, 1.5)),
    "betag_range": (0.5, 4.0),
    "betap_range": (1.0, 2.0),
    "blur_prob": (1.0, 0.8),                         # (the first blur always runs; second_blur_prob)
    "resize_prob": ((0.2, 0.7, 0.1), (0.3, 0.4, 0.3)),          # up, down, keep
    "resize_range": ((0.15, 1.5), (0.3, 1.2)),
    "noise_range": ((1.0, 30.0), (1.0, 25.0)),
    "gray_noise_prob": (0.4, 0.4),
    "jpeg_range": ((30.0, 95.0), (30.0, 95.0)),
    "final_sinc_prob": 0.8,
    "resize_filters": ("bilinear", "bilinear", "bicubic"),      # the reference's area / bilinear / bicubic; "area" -> bilinear
}


# ---- blur kernels (fp64, sum 1) ---------------------------------------------------------------------------------------------
def _check_ksize(ksize):
    if isinstance(ksize, bool) or int(ksize) != ksize or ksize < 1 or ksize % 2 != 1 or ksize > KSIZE_MAX:
        raise ValueError(f"kernel size must be odd, in [1, {KSIZE_MAX}], got {ksize!r}")
    return int(ksize)


def _quadratic_form(ksize, sigma_x, sigma_y, theta):
    """g^T S^-1 g on the ksize x ksize grid centred at 0, S = R(theta) diag(sigma_x^2, sigma_y^2) R(theta)^T"""
    if not (sigma_x > 0 and sigma_y > 0):
        raise ValueError(f"sigma_x and sigma_y must be positive, got {sigma_x!r}, {sigma_y!r}")
    r = _check_ksize(ksize) // 2
    y, x = np.meshgrid(np.arange(-r, r + 1, dtype=np.float64), np.arange(-r, r + 1, dtype=np.float64), indexing="ij")
    c, s = math.cos(theta), math.sin(theta)
    u, v = c * x + s * y, -s * x + c * y
    return (u / sigma_x) ** 2 + (v / sigma_y) ** 2


def _normalised(k):
    return k / k.sum()


def gaussian_kernel(ksize, sigma_x, sigma_y=None, theta=0.0):
    """exp(-q / 2), q = g^T S^-1 g: isotropic when sigma_y is None, else anisotropic and rotated by theta"""
    return _normalised(np.exp(-0.5 * _quadratic_form(ksize, sigma_x, sigma_x if sigma_y is None else sigma_y, theta)))


def generalized_gaussian_kernel(ksize, sigma_x, beta, sigma_y=None, theta=0.0):
    """exp(-q^beta / 2)"""
    return _normalised(np.exp(-0.5 * _quadratic_form(ksize, sigma_x, sigma_x if sigma_y is None else sigma_y, theta) ** beta))


def plateau_kernel(ksize, sigma_x, beta, sigma_y=None, theta=0.0):
    """1 / (1 + q^beta)"""
    return _normalised(1.0 / (1.0 + _quadratic_form(ksize, sigma_x, sigma_x if sigma_y is None else sigma_y, theta) ** beta))


_J1_NODES = 128


def bessel_j1(x):
    """J1(x) = (1 / pi) int_0^pi cos(tau - x sin tau) d tau by the midpoint rule on 128 nodes: the integrand is smooth and its
    odd derivatives agree at the two ends, so the rule converges geometrically; |error| < 1e-13 for |x| <= 64 (the largest
    argument of a 21 x 21 kernel is pi * 10 * sqrt(2) < 45)."""
    x = np.asarray(x, dtype=np.float64)
    tau = (np.arange(_J1_NODES, dtype=np.float64) + 0.5) * (math.pi / _J1_NODES)
    return np.cos(tau - x[..., None] * np.sin(tau)).mean(axis=-1)


def sinc_kernel(ksize, omega_c):
    """The circular low-pass filter of cutoff omega_c (radians per pixel): omega_c J1(omega_c rho) / (2 pi rho), rho the distance
    from the centre, omega_c^2 / (4 pi) at the centre"""
    if not 0 < omega_c <= math.pi:
        raise ValueError(f"omega_c must be in (0, pi], got {omega_c!r}")
    r = _check_ksize(ksize) // 2
    y, x = np.meshgrid(np.arange(-r, r + 1, dtype=np.float64), np.arange(-r, r + 1, dtype=np.float64), indexing="ij")
    rho = np.sqrt(x * x + y * y)
    safe = np.where(rho > 0, rho, 1.0)
    k = np.where(rho > 0, omega_c * bessel_j1(omega_c * safe) / (2.0 * math.pi * safe), omega_c * omega_c / (4.0 * math.pi))
    return _normalised(k)


def pad_kernel(k, size=KSIZE_MAX):
    """zero-pad a smaller odd kernel into the centre of a size x size one"""
    k = np.asarray(k, dtype=np.float64)
    if k.ndim != 2 or k.shape[0] != k.shape[1] or k.shape[0] % 2 != 1 or k.shape[0] > _check_ksize(size):
        raise ValueError(f"pad_kernel: an odd square kernel of at most {size} x {size} is needed, got {k.shape}")
    p = (size - k.shape[0]) // 2
    return np.pad(k, ((p, p), (p, p)))


# ---- recipes ----------------------------------------------------------------------------------------------------------------
def _kernel_or_none(k):
    if k is None:
        return None
    k = np.asarray(k, dtype=np.float64)
    if k.ndim != 2 or k.shape[0] != k.shape[1]:
        raise ValueError(f"a blur kernel must be square, got {k.shape}")
    _check_ksize(k.shape[0])
    return k


@dataclasses.dataclass
class Stage:
    """One round of the chain, in this order; a part that is None / 0 is skipped.
      blur           k x k fp64 kernel (k odd, <= 21) or None
      scale          the size after this stage as a factor of the INPUT image's size: (int(H scale), int(W scale))
      resize_filter  "bilinear", "bicubic" or "lanczos" (PIL's definitions, antialiased)
      noise_sigma    Gaussian noise in 0..255 units; 0: none
      gray_noise     one noise value per pixel instead of one per channel
      jpeg_quality   in [1, 99]; 0: none"""
    blur: Optional[np.ndarray] = None
    scale: float = 1.0
    resize_filter: str = "bicubic"
    noise_sigma: float = 0.0
    gray_noise: bool = False
    jpeg_quality: float = 0.0

    def __post_init__(self):
        from .resample import FILTERS
        self.blur = _kernel_or_none(self.blur)
        self.scale, self.noise_sigma, self.jpeg_quality = float(self.scale), float(self.noise_sigma), float(self.jpeg_quality)
        self.gray_noise = bool(self.gray_noise)
        if self.resize_filter not in FILTERS:
            raise ValueError(f"Stage: resize_filter must be one of {FILTERS}, got {self.resize_filter!r}")
        if not 0 < self.scale <= 8:
            raise ValueError(f"Stage: scale must be in (0, 8], got {self.scale}")
        if not 0 <= self.noise_sigma <= 255:
            raise ValueError(f"Stage: noise_sigma must be in [0, 255], got {self.noise_sigma}")
        if self.jpeg_quality != 0 and not 1 <= self.jpeg_quality <= 99:
            raise ValueError(f"Stage: jpeg_quality must be 0 (none) or in [1, 99], got {self.jpeg_quality}")


@dataclasses.dataclass
class Recipe:
    """stages, then the resize to (H // sf, W // sf) with `final_filter` followed by the `final_sinc` kernel (None: no filter);
    the last stage's JPEG runs before that resize when `jpeg_before_final_resize`, after the sinc filter otherwise; with
    `resize_lq` the result goes back to (H, W) with bicubic (utils/degradation_pipeline.py:330-336).  Values are clamped to
    [0, 1] at the end."""
    stages: List[Stage] = dataclasses.field(default_factory=list)
    final_sinc: Optional[np.ndarray] = None
    jpeg_before_final_resize: bool = False
    sf: int = 4
    resize_lq: bool = True
    final_filter: str = "bicubic"

    def __post_init__(self):
        from .resample import FILTERS
        self.stages = [s if isinstance(s, Stage) else Stage(**s) for s in self.stages]
        self.final_sinc = _kernel_or_none(self.final_sinc)
        self.jpeg_before_final_resize, self.resize_lq = bool(self.jpeg_before_final_resize), bool(self.resize_lq)
        if isinstance(self.sf, bool) or int(self.sf) != self.sf or not 1 <= self.sf <= 16:
            raise ValueError(f"Recipe: sf must be an integer in [1, 16], got {self.sf!r}")
        self.sf = int(self.sf)
        if self.final_filter not in FILTERS:
            raise ValueError(f"Recipe: final_filter must be one of {FILTERS}, got {self.final_filter!r}")

    def to_json(self):
        d = dataclasses.asdict(self)
        for holder in [d] + d["stages"]:
            for key in ("blur", "final_sinc"):
                if holder.get(key) is not None:
                    holder[key] = np.asarray(holder[key]).tolist()         # (repr of a float64 reads back to the same bits)
        return json.dumps(d, indent=1, sort_keys=True)

    @classmethod
    def from_json(cls, text):
        d = json.loads(text)
        if not isinstance(d, dict) or "stages" not in d:
            raise ValueError("not a degradation recipe: a JSON object with a \"stages\" list is needed")
        return cls(**d)

    def __eq__(self, other):
        return isinstance(other, Recipe) and self.to_json() == other.to_json()


def _rng(seed, name):
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 1 << 64:
        raise ValueError(f"seed must be an integer in [0, 2^64), got {seed!r}")
    return np.random.Generator(np.random.Philox(key=np.array([seed, zlib.crc32(str(name).encode("utf-8"))], dtype=np.uint64)))


def noise_seed(seed, name=""):
    """The seed of a file's noise launches: (seed, crc32(name)) folded into 64 bits, so that a file's noise does not depend on
    which batch or rank it falls into"""
    _rng(seed, name)
    return ((seed ^ (seed >> 32)) & 0xffffffff) | (zlib.crc32(str(name).encode("utf-8")) << 32)


def _draw_kernel(g, opt, stage):
    ksize = int(g.choice(KERNEL_SIZES))
    if g.uniform() < opt["sinc_prob"][stage]:
        return sinc_kernel(ksize, g.uniform(math.pi / 3 if ksize < 13 else math.pi / 5, math.pi))     # :117-121
    kind = KERNEL_KINDS[int(g.choice(len(KERNEL_KINDS), p=opt["kernel_prob"]))]
    lo, hi = opt["blur_sigma"][stage]
    sx = g.uniform(lo, hi)
    sy, theta = (g.uniform(lo, hi), g.uniform(-math.pi, math.pi)) if kind.endswith("aniso") else (None, 0.0)
    if kind.startswith("generalized"):
        return generalized_gaussian_kernel(ksize, sx, g.uniform(*opt["betag_range"]), sy, theta)
    if kind.startswith("plateau"):
        return plateau_kernel(ksize, sx, g.uniform(*opt["betap_range"]), sy, theta)
    return gaussian_kernel(ksize, sx, sy, theta)


def sample_recipe(preset, seed, name="", sf=4, resize_lq=True):
    """A recipe as a pure function of (preset, seed, name): every choice comes from numpy.random.Generator(Philox(key =
    (seed, crc32(name)))), so a file's recipe depends neither on batch order nor on how ranks shard the list.

    "bicubic": one bicubic downsample by sf and nothing else, the classic super-resolution protocol.
    "realesrgan": the second-order chain with the ranges and probabilities of utils/degradation_pipeline.py:20-64 (kernel sizes
    7..21, six kernel families or a sinc kernel, resize up / down / keep, noise, JPEG 30..95, twice; the final sinc filter
    with probability 0.8 and either order of the last JPEG and the final resize).  Deviations from the reference: Gaussian
    noise is drawn where it would draw Poisson noise (half of the time); the resize filters are PIL's antialiased bilinear /
    bicubic, with its "area" mapped to bilinear; no USM sharpening of the ground truth; no 1 % no-degradation pass-through;
    and the draw order is this function's, not that of Python's `random`."""
    if preset not in PRESETS:
        raise ValueError(f"unknown degradation preset {preset!r}: one of {PRESETS}")
    g = _rng(seed, name)
    if preset == "bicubic":
        return Recipe([Stage(scale=1.0 / sf, resize_filter="bicubic")], sf=sf, resize_lq=resize_lq, final_filter="bicubic")
    opt, stages = REALESRGAN, []
    for i in range(2):
        blur = _draw_kernel(g, opt, i)                                   # (drawn even when unused: later draws keep their place)
        if not g.uniform() < opt["blur_prob"][i]:
            blur = None
        mode = int(g.choice(3, p=opt["resize_prob"][i]))
        lo, hi = opt["resize_range"][i]
        up, down = g.uniform(1.0, hi), g.uniform(lo, 1.0)
        scale = (up, down, 1.0)[mode] / (1 if i == 0 else sf)
        stages.append(Stage(blur=blur, scale=scale, resize_filter=opt["resize_filters"][int(g.integers(3))],
                            noise_sigma=g.uniform(*opt["noise_range"][i]), gray_noise=bool(g.uniform() < opt["gray_noise_prob"][i]),
                            jpeg_quality=g.uniform(*opt["jpeg_range"][i])))
    final = sinc_kernel(int(g.choice(KERNEL_SIZES)), g.uniform(math.pi / 3, math.pi))
    if not g.uniform() < opt["final_sinc_prob"]:
        final = None
    return Recipe(stages, final_sinc=final, jpeg_before_final_resize=bool(g.uniform() < 0.5), sf=sf, resize_lq=resize_lq,
                  final_filter=opt["resize_filters"][int(g.integers(3))])


def load_recipe(spec, seed=0, name=""):
    """`spec`: a preset name (sampled with (seed, name)) or the path of a recipe JSON file"""
    if spec in PRESETS:
        return sample_recipe(spec, seed, name)
    try:
        with open(spec) as f:
            return Recipe.from_json(f.read())
    except (OSError, ValueError, TypeError) as e:
        raise ValueError(f"{spec!r} is neither a preset {PRESETS} nor a readable recipe JSON: {e}") from None


# ---- the chain --------------------------------------------------------------------------------------------------------------
def _shared(recipes, what, values):
    if len(set(values)) != 1:
        raise ValueError(f"degrade: the recipes of one batch must share {what}, got {sorted(set(values), key=str)}")
    return values[0]


def _batch_taps(kernels, device):
    """per-image kernels (None: the identity) padded to the batch's largest size -> fp32 (N, k, k) on the device"""
    k = max(1 if b is None else b.shape[0] for b in kernels)
    pulse = np.zeros((1, 1))
    pulse[0, 0] = 1.0
    return torch.from_numpy(np.stack([pad_kernel(pulse if b is None else b, k) for b in kernels]).astype(np.float32)).to(device)


def degrade(images, recipe, seed=0, device=None, return_stages=False):
    """Clean images -> low-quality ones on the device.  `images`: PIL image(s), uint8 (N, H, W, 3) / float (N, 3, H, W) arrays or
    tensors (resample.as_batch); `recipe`: one Recipe for the batch or a list with one per image -- per-image kernels, sigmas
    and qualities then go into single launches, while everything that shapes the tensors (the stage count, which parts run,
    resize factors and filters, gray noise, sf, the JPEG order) must be shared; `seed`: of the noise (stage i of the chain is
    noise stream i; the image's index in the batch is part of the counter).  Returns fp32 (N, 3, h, w) in [0, 1] on the
    device; with `return_stages` also the list of (label, tensor) of every intermediate result, in order."""
    from . import ops
    from .resample import as_batch
    batch, kind = as_batch(images)
    if device is None:
        device = batch.device if torch.is_tensor(batch) and batch.is_cuda else torch.device("cuda:0")
    src = (batch if torch.is_tensor(batch) else torch.from_numpy(batch)).to(device)
    x = src.permute(0, 3, 1, 2).to(torch.float32).div_(255.0).contiguous() if kind == "u8" else src.to(torch.float32).contiguous()
    N, Cc, H, W = x.shape
    if Cc != 3:
        raise ValueError(f"degrade: RGB images are needed, got {Cc} channel(s)")
    recipes = list(recipe) if isinstance(recipe, (list, tuple)) else [recipe] * N
    if len(recipes) != N or not all(isinstance(r, Recipe) for r in recipes):
        raise ValueError(f"degrade: one Recipe, or a list of one per image ({N}), is needed")
    nst = _shared(recipes, "the number of stages", [len(r.stages) for r in recipes])
    sf = _shared(recipes, "sf", [r.sf for r in recipes])
    resize_lq = _shared(recipes, "resize_lq", [r.resize_lq for r in recipes])
    jpeg_first = _shared(recipes, "jpeg_before_final_resize", [r.jpeg_before_final_resize for r in recipes])
    final_filter = _shared(recipes, "final_filter", [r.final_filter for r in recipes])
    trace = []

    def keep(label, t):
        trace.append((label, t))
        return t

    def blur(t, kernels, label):
        if all(b is None for b in kernels):
            return t
        taps = _batch_taps(kernels, device)
        r = (taps.shape[-1] - 1) // 2
        if min(t.shape[-2:]) <= r:
            raise ValueError(f"degrade: {label}: a {taps.shape[-1]} x {taps.shape[-1]} kernel needs an image larger than {r} pixels per "
                             f"side, got {t.shape[-2]}x{t.shape[-1]}")
        return keep(label, ops.filter2d(t, taps))

    def resize(t, size, flt, label):
        size = (max(1, size[0]), max(1, size[1]))
        return t if tuple(t.shape[-2:]) == size else keep(label, ops.resample(t, size, flt))

    def jpeg(t, i):
        return keep(f"stage{i}.jpeg", ops.jpeg_roundtrip(t, [r.stages[i].jpeg_quality for r in recipes]))

    last_jpeg = None
    for i in range(nst):
        st = [r.stages[i] for r in recipes]
        x = blur(x, [s.blur for s in st], f"stage{i}.blur")
        scale = _shared(recipes, f"stage {i}'s scale", [s.scale for s in st])
        x = resize(x, (int(H * scale), int(W * scale)), _shared(recipes, f"stage {i}'s resize_filter", [s.resize_filter for s in st]),
                   f"stage{i}.resize")
        if any(s.noise_sigma > 0 for s in st):
            gray = _shared(recipes, f"stage {i}'s gray_noise", [s.gray_noise for s in st if s.noise_sigma > 0])
            x = keep(f"stage{i}.noise", ops.add_gaussian_noise(x, [s.noise_sigma for s in st], seed, stream=i, gray=gray))
        if _shared(recipes, f"whether stage {i} has a JPEG pass", [s.jpeg_quality > 0 for s in st]):
            if i == nst - 1 and not jpeg_first:
                last_jpeg = i
            else:
                x = jpeg(x, i)
    x = resize(x, (H // sf, W // sf), final_filter, "final.resize")
    x = blur(x, [r.final_sinc for r in recipes], "final.sinc")
    if last_jpeg is not None:
        x = jpeg(x, last_jpeg)
    size = (H, W) if resize_lq else tuple(x.shape[-2:])
    x = keep("out", ops.resample(x, size, "bicubic", clamp=(0.0, 1.0)))       # (equal sizes: the clamp alone)
    return (x, trace) if return_stages else x


def quantize_u8(lq):
    """fp32 (N, 3, h, w) in [0, 1] -> uint8 (N, h, w, 3) on the host: floor(255 v + 0.5), the 8-bit image that gets saved"""
    return torch.floor(lq.detach().to("cpu", torch.float32) * 255.0 + 0.5).clamp_(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous().numpy()
