"""PSNR and SSIM of restored images on the device (an addition: the reference's `losses/` covers the training side only).

The definitions are the ones restoration papers report (basicsr's `calculate_psnr` / `calculate_ssim`; DESIGN.md section 7
"Image metrics"), the arithmetic is one launch pair of `ops.image_metrics` per call, and what comes back are Python floats:

    from instantir_amd import metrics
    metrics.psnr(restored, gt)                       # a float for one image, a list for a batch
    metrics.evaluate(restored, gt, crop_border=4, y_channel=True)
    metrics.input_fidelity(restored, lq)             # no ground truth: how far did the restoration move from its input

Images are what the pipeline returns and what a user has: a PIL image or a list of them, a uint8 numpy array (H, W), (H, W, C)
or (N, H, W, C), a float numpy array of the same layouts on a [0, 1] scale (`output_type="np"`), a uint8 tensor in those
layouts, or a float tensor (C, H, W) / (N, C, H, W) on a [0, 1] scale (`output_type="pt"`).  An 8-bit source is uploaded as
uint8.  There is no host path: without the library and a GPU the calls raise.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from .images import check_crop, dims, host_source, scoring_device

METRICS = ("psnr", "ssim")
WINDOW = 11


def _check_options(who, what, crop_border, y_channel, quantize):
    names = (what,) if isinstance(what, str) else tuple(what)
    if not names or any(w not in METRICS for w in names):
        raise ValueError(f"{who}: metrics must name one or both of {METRICS}, got {what!r}")
    check_crop(who, crop_border)
    if isinstance(quantize, (bool, np.bool_)):
        quantize = (bool(quantize), bool(quantize))
    try:
        qa, qb = (bool(q) for q in quantize)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: quantize must be a flag or a pair of flags (for a, for b), got {quantize!r}") from None
    return tuple(n for n in METRICS if n in names), (qa, qb)


def _check_pair(who, ta, tb, names, crop_border, y_channel, arg_b="b"):
    da, db = dims(ta), dims(tb)
    if da != db:
        raise ValueError(f"{who}: {arg_b} is (N, C, H, W) = {db} but its counterpart is {da}")
    N, C, H, W = da
    if C not in (1, 3):
        raise ValueError(f"{who}: a and b must have 1 or 3 channels, got {C}")
    if y_channel and C != 3:
        raise ValueError(f"{who}: y_channel needs 3 channels, got {C}")
    side = WINDOW if "ssim" in names else 1
    if min(H, W) - 2 * crop_border < side:
        raise ValueError(f"{who}: crop_border {crop_border} leaves less than {side} pixel(s) per side of {H}x{W}"
                         + (" (the SSIM window is 11 x 11)" if "ssim" in names else ""))


def psnr_from_mse(mse):
    """10 log10(255^2 / MSE) in fp64; inf for identical images."""
    return math.inf if mse == 0 else 10.0 * math.log10(255.0 ** 2 / mse)


def _score(ta, tb, names, crop_border, y_channel, quantize, device):
    from . import ops
    dev = scoring_device(device)
    out = ops.image_metrics(ta.to(dev).contiguous(), tb.to(dev).contiguous(), crop_border=crop_border, y_channel=bool(y_channel),
                            quantize=quantize, what=names).cpu().tolist()
    res = {}
    if "psnr" in names:
        res["psnr"] = [psnr_from_mse(row[0]) for row in out]
    if "ssim" in names:
        res["ssim"] = [float(row[1]) for row in out]
    return res


def _run(who, a, b, names, crop_border, y_channel, quantize, device):
    names, quantize = _check_options(who, names, crop_border, y_channel, quantize)
    ta, single_a = host_source(a, "a")
    tb, single_b = host_source(b, "b")
    _check_pair(who, ta, tb, names, crop_border, y_channel)
    return _score(ta, tb, names, crop_border, y_channel, quantize, device), single_a and single_b


def psnr(a, b, crop_border=0, y_channel=False, quantize=False, device=None):
    """PSNR in dB of `a` against `b`: a float for one image, a list of floats for a batch; inf for identical images."""
    res, single = _run("psnr", a, b, ("psnr",), crop_border, y_channel, quantize, device)
    return res["psnr"][0] if single else res["psnr"]


def ssim(a, b, crop_border=0, y_channel=False, quantize=False, device=None):
    """SSIM (11 x 11 Gaussian window, sigma 1.5, valid positions only) of `a` against `b`: a float or a list of floats."""
    res, single = _run("ssim", a, b, ("ssim",), crop_border, y_channel, quantize, device)
    return res["ssim"][0] if single else res["ssim"]


def _with_means(res):
    for name in list(res):
        res[name + "_mean"] = float(sum(res[name]) / len(res[name]))
    return res


def _model_scores(who, a, b, model, device, name):
    d = None if device is None else torch.device(device)
    if d is not None and (d.type != model.device.type or (d.index is not None and d.index != model.device.index)):
        raise ValueError(f"{who}: the {name.upper()} model lives on {model.device}, not on {d}")
    return model(a, b).cpu().tolist()


def _add_model_scores(res, who, a, b, device, lpips_model, dists_model):
    """`res` with the per-image scores of the pair models that were given, "lpips" before "dists", and every mean."""
    for name, model in (("lpips", lpips_model), ("dists", dists_model)):
        if model is not None:
            res[name] = _model_scores(who, a, b, model, device, name)
    return _with_means(res)


def _model_metric(name, a, b, model, device):
    _, single_a = host_source(a, "a")
    _, single_b = host_source(b, "b")
    out = _model_scores(name, a, b, model, device, name)
    return out[0] if single_a and single_b else out


def lpips(a, b, model, device=None):
    """LPIPS of `a` against `b` under `model` (an `instantir_amd.lpips.LPIPS`; DESIGN.md section 7 "LPIPS"): a float for one
    image, a list of floats for a batch; 0 for identical images.  The whole image is scored: LPIPS has no crop, luma or
    quantise option."""
    return _model_metric("lpips", a, b, model, device)


def dists(a, b, model, device=None):
    """DISTS of `a` against `b` under `model` (an `instantir_amd.dists.DISTS`; DESIGN.md section 7 "DISTS"): a float for one
    image, a list of floats for a batch; 0 for identical images.  The whole image is scored, as for LPIPS."""
    return _model_metric("dists", a, b, model, device)


def niqe(images, model, crop_border=0, device=None):
    """NIQE of `images` under `model` (an `instantir_amd.niqe.NIQE`; DESIGN.md section 7 "NIQE"): no second image is needed.  A
    float for one image, a list of floats for a batch; lower is better.  C = 3 is scored on its BT.601 luma."""
    _, single = host_source(images, "images")
    out = model(images, crop_border=crop_border, device=device).tolist()
    return out[0] if single else out


def evaluate(a, b, metrics=METRICS, crop_border=0, y_channel=False, quantize=False, device=None, lpips_model=None, dists_model=None):
    """Both figures in one launch pair: {"psnr": [per image], "ssim": [per image], "psnr_mean": .., "ssim_mean": ..} (only the
    metrics asked for).  `quantize` (a flag, or one per argument) rounds a float source to the 8-bit image that would be saved.
    With an `lpips_model` the result gains "lpips" and "lpips_mean" (of the whole, uncropped RGB images), with a `dists_model`
    "dists" and "dists_mean" likewise."""
    res, _ = _run("evaluate", a, b, metrics, crop_border, y_channel, quantize, device)
    return _add_model_scores(res, "evaluate", a, b, device, lpips_model, dists_model)


def input_fidelity(restored, lq, filter="bicubic", metrics=METRICS, crop_border=0, y_channel=False, device=None, lpips_model=None,
                   dists_model=None):
    """How far the restoration moved from what it was given: `restored` is brought to the size of `lq` with `ops.resample`
    (PIL's `filter`; quantised mode when both are 8-bit, untouched at equal sizes) and scored against `lq`.  Returns what
    `evaluate` returns ("lpips" / "dists" included when an `lpips_model` / a `dists_model` is given: of the resized restoration
    against `lq`)."""
    from . import ops
    from .resample import FILTERS
    if filter not in FILTERS:
        raise ValueError(f"input_fidelity: filter must be one of {tuple(FILTERS)}, got {filter!r}")
    names, _ = _check_options("input_fidelity", metrics, crop_border, y_channel, False)
    tr, _ = host_source(restored, "restored")
    tl, _ = host_source(lq, "lq")
    dr, dl = dims(tr), dims(tl)
    if dr[:2] != dl[:2]:
        raise ValueError(f"input_fidelity: restored holds (N, C) = {dr[:2]} but lq {dl[:2]}")
    quantize = (False, False)
    dev = scoring_device(device) if dr[2:] != dl[2:] else None
    if dr[2:] != dl[2:]:
        both_u8 = tr.dtype == torch.uint8 and tl.dtype == torch.uint8
        if tr.dtype == torch.uint8:
            tr = ops.resample(tr.to(dev), dl[2:], filter, quantize=both_u8, scale=1.0 / 255.0)
        else:
            tr = ops.resample(tr.to(dev).contiguous(), dl[2:], filter, clamp=(0.0, 1.0))
        quantize = (both_u8, False)
    _check_pair("input_fidelity", tr, tl, names, crop_border, y_channel, arg_b="lq")
    res = _score(tr, tl, names, crop_border, y_channel, quantize, dev if dev is not None else device)
    return _add_model_scores(res, "input_fidelity", tr, tl, device, lpips_model, dists_model)
