"""Command line restoration driver with the flags and behaviour of the reference's `infer.py`:

    python -m instantir_amd.infer --sdxl_path SDXL --vision_encoder_path DINOV2 --instantir_path INSTANTIR \\
        --test_path INPUTS --out_path OUT [--cfg 7.0 --preview_start 0.0 --creative_start 1.0 ...]

Mirrors: model assembly `infer.py:114-144`, batching + skip-done logic :148-169, `resize_img` :31-66, default
prompts :192-205 (byte for byte: the backslash continuations put the runs of spaces INSIDE the prompt text,
SURVEY.md Appendix C Q10), the pipeline call :211-222, resize-back + save :224-225.  `--denoising_start` is accepted
and has no effect on the schedule, as in the reference (Q1).  Flags the reference parses but never uses
(`--adapter_tokens --resolution --variant --revision --pretrained_vae_model_name_or_path`) are accepted too.

Extension (not in the reference): `--synthetic {tiny,sdxl}` builds every network from seeded synthetic weights so the
driver can be exercised without checkpoints (none are available offline); with it the text prompt is replaced by
seeded embeddings because no tokenizer vocabulary exists here.  `--apg ETA NORM_THRESHOLD MOMENTUM` turns adaptive projected
guidance on (`pipe.enable_apg(...)`: the CFG update's saturating parallel part down-weighted, its norm clamped, with momentum).
`--gt_path DIR` scores every saved image against the file of the same name in DIR (PSNR / SSIM on the device,
`instantir_amd.metrics`), `--input_fidelity` against its own input file; the figures go to `metrics.json` in the output directory.
`--lpips_path PATH [--lpips_lin_path PATH]` adds LPIPS (VGG-16, `instantir_amd.lpips`) to each scored pair.
`--dists_path PATH [--dists_weights_path PATH]` adds DISTS (VGG-16 with L2 pooling, `instantir_amd.dists`) likewise.
`--niqe_path PARAMS` scores every saved image with NIQE (`instantir_amd.niqe`), which needs no second image.
`--degrade PRESET_OR_JSON [--degrade_seed N]` treats the files of `--test_path` as clean images: each is degraded on the device
(`instantir_amd.degrade`), the 8-bit result stands in for the file that was read and is saved with its recipe under `lq/` in the
output directory, and unless told otherwise the run scores its restorations against the clean files.
"""
from __future__ import annotations

import argparse
import os

import numpy as np
import torch
from PIL import Image

DEFAULT_PROMPT = "Photorealistic, highly detailed, hyper detailed photo - realistic maximum detail, 32k, \
                ultra HD, extreme meticulous detailing, skin pore detailing, \
                hyper sharpness, perfect without deformations, \
                taken using a Canon EOS R camera, Cinematic, High Contrast, Color Grading. "
DEFAULT_NEG_PROMPT = "blurry, out of focus, unclear, depth of field, over-smooth, \
                sketch, oil painting, cartoon, CG Style, 3D render, unreal engine, \
                dirty, messy, worst quality, low quality, frames, painting, illustration, drawing, art, \
                watermark, signature, jpeg artifacts, deformed, lowres"


def resize_plan(size, max_side=1024, min_side=768, width=None, height=None, base_pixel_number=64):
    """The sizes of infer.py:31-66 for an input of `size` = (w, h): requested output size, then min side -> 768, max side ->
    1024, floor to a multiple of 64.  Returns ((work_w, work_h), (out_w, out_h))."""
    w, h = size
    if width is not None and height is not None:
        out_w, out_h = width, height
    elif width is not None:
        out_w, out_h = width, round(h * width / w)
    elif height is not None:
        out_w, out_h = round(w * height / h), height
    else:
        out_w, out_h = w, h
    w, h = out_w, out_h
    if min(w, h) < min_side:
        r = min_side / min(w, h)
        w, h = round(r * w), round(r * h)
    if max(w, h) > max_side:
        r = max_side / max(w, h)
        w, h = round(r * w), round(r * h)
    return ((w // base_pixel_number) * base_pixel_number, (h // base_pixel_number) * base_pixel_number), (out_w, out_h)


def resize_img(input_image, max_side=1024, min_side=768, width=None, height=None, pad_to_max_side=False,
               mode=Image.BILINEAR, base_pixel_number=64):
    """infer.py:31-66: the sizes of `resize_plan`, the resize with PIL on the host.
    Returns (resized image, (out_w, out_h)) -- the second item is what the result is resized back to."""
    (wn, hn), (out_w, out_h) = resize_plan(input_image.size, max_side, min_side, width, height, base_pixel_number)
    input_image = input_image.resize([wn, hn], mode)
    if pad_to_max_side:
        canvas = np.ones([max_side, max_side, 3], dtype=np.uint8) * 255
        ox, oy = (max_side - wn) // 2, (max_side - hn) // 2
        canvas[oy:oy + hn, ox:ox + wn] = np.array(input_image)
        input_image = Image.fromarray(canvas)
    return input_image, (out_w, out_h)


def plan_batches(test_path, out_dir, batch_size):
    """infer.py:148-169: sorted inputs, files already present in the output directory are skipped."""
    done = set(os.listdir(out_dir))
    names = [test_path.split("/")[-1]] if os.path.isfile(test_path) else sorted(os.listdir(test_path))
    batches, cur = [], []
    for f in sorted(names):
        if f in done:
            print(f"Skip {f}")
            continue
        cur.append(f)
        if len(cur) == batch_size:
            batches.append(cur)
            cur = []
    if cur:
        batches.append(cur)
    return batches


def shard_batches(batches, rank, world):
    """Multi-GPU: the batch list infer.py:151-169 forms is cut into contiguous per-rank slices;
    images never interact, so each rank runs the whole loop on its slice and there is no per-step collective."""
    from .parallel import shard_range
    lo, hi = shard_range(len(batches), rank, world)
    return batches[lo:hi]


# --scheduler choice -> (class in instantir_amd.schedulers, from_config overrides)
SCHEDULERS = {
    "ddpm": ("DDPMScheduler", {}),
    "ddim": ("DDIMScheduler", {}),
    "euler": ("EulerDiscreteScheduler", {}),
    "euler_a": ("EulerAncestralDiscreteScheduler", {}),
    "dpmpp_2m": ("DPMSolverMultistepScheduler", {"algorithm_type": "dpmsolver++"}),
    "dpmpp_2m_sde": ("DPMSolverMultistepScheduler", {"algorithm_type": "sde-dpmsolver++"}),
}


def build_parser():
    p = argparse.ArgumentParser(description="InstantIR restoration on MI355X")
    p.add_argument("--sdxl_path", type=str, default=None)
    p.add_argument("--previewer_lora_path", type=str, default=None)
    p.add_argument("--pretrained_vae_model_name_or_path", type=str, default=None)
    p.add_argument("--instantir_path", type=str, default=None)
    p.add_argument("--vision_encoder_path", type=str, default="/share/huangrenyuan/model_zoo/vis_backbone/dinov2_large")
    p.add_argument("--adapter_model_path", type=str, default=None)
    p.add_argument("--adapter_tokens", type=int, default=64)
    p.add_argument("--use_clip_encoder", action="store_true")
    p.add_argument("--denoising_start", type=int, default=1000)
    p.add_argument("--num_inference_steps", type=int, default=30)
    p.add_argument("--creative_start", type=float, default=1.0)
    p.add_argument("--preview_start", type=float, default=0.0)
    p.add_argument("--resolution", type=int, default=1024)
    p.add_argument("--batch_size", type=int, default=6)
    p.add_argument("--width", type=int, default=None)
    p.add_argument("--height", type=int, default=None)
    p.add_argument("--cfg", type=float, default=7.0)
    p.add_argument("--post_fix", type=str, default=None)
    p.add_argument("--variant", type=str, default="fp16")
    p.add_argument("--revision", type=str, default=None, required=False)
    p.add_argument("--prompt", type=str, default="", nargs="+")
    p.add_argument("--neg_prompt", type=str, default="", nargs="+")
    p.add_argument("--test_path", type=str, default=None, required=True)
    p.add_argument("--out_path", type=str, default="./output")
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--synthetic", choices=["tiny", "sdxl"], default=None, help="seeded synthetic weights (no checkpoints needed)")
    p.add_argument("--freeu", type=float, nargs=4, default=None, metavar=("S1", "S2", "B1", "B2"),
                   help="FreeU factors (pipe.enable_freeu(s1, s2, b1, b2)); off by default. SDXL: 0.9 0.2 1.3 1.4")
    p.add_argument("--scheduler", choices=sorted(SCHEDULERS), default="ddpm",
                   help="main scheduler, built as Cls.from_config(pipe.scheduler.config); default ddpm (the reference's)")
    p.add_argument("--karras", action="store_true", help="Karras sigmas (use_karras_sigmas=True) for euler / dpmpp_2m / dpmpp_2m_sde")
    p.add_argument("--pag_scale", type=float, default=0.0,
                   help="perturbed-attention guidance scale; 0 (default) = off, > 0 calls pipe.enable_pag(--pag_layers)")
    p.add_argument("--pag_adaptive_scale", type=float, default=0.0,
                   help="PAG adaptive scale: s_t = max(pag_scale - pag_adaptive_scale * (1000 - t), 0)")
    p.add_argument("--pag_layers", type=str, default="mid",
                   help="comma-separated PAG layer expressions over the UNet's self-attention names (default mid), e.g. mid,up_blocks.0")
    p.add_argument("--seg_scale", type=float, default=0.0,
                   help="smoothed-energy guidance scale; 0 (default) = off, > 0 calls pipe.enable_seg(--seg_layers, --seg_blur_sigma)")
    p.add_argument("--seg_blur_sigma", type=float, default=100.0,
                   help="SEG: sigma of the Gaussian blur of the perturbed rows' queries, in tokens (default 100; inf = the mean query)")
    p.add_argument("--seg_layers", type=str, default="mid",
                   help="comma-separated SEG layer expressions over the UNet's self-attention names (default mid), e.g. mid,up_blocks.0")
    p.add_argument("--apg", type=float, nargs=3, default=None, metavar=("ETA", "NORM_THRESHOLD", "MOMENTUM"),
                   help="adaptive projected guidance (pipe.enable_apg(eta, norm_threshold, momentum)); off by default. "
                        "The pipeline's defaults: 0.0 15.0 -0.5")
    p.add_argument("--color_fix", choices=["none", "wavelet", "adain"], default="none",
                   help="transfer the colour of the LQ input onto the restored image after the VAE decode (pipe(..., color_fix=...)); "
                        "default none")
    p.add_argument("--vae_flash_attention", action="store_true",
                   help="run the VAE mid-block attention as one flash-style launch (pipe.vae.enable_flash_attention()): untiled "
                        "encode / decode beyond 1024x1024; off by default")
    p.add_argument("--restore_map", type=str, default=None, metavar="PATH",
                   help="per-pixel restoration strength (pipe(..., restore_map=...)): a grey-scale image file used for every input, or "
                        "a directory holding one map per input file name; white = restore freely, black = keep the input pixels")
    p.add_argument("--map_feather", type=int, default=4, help="half width in pixels of the seam between kept and restored pixels "
                                                              "(pipe(..., map_feather=N)); 0 = hard paste; default 4")
    p.add_argument("--device_resize", action="store_true",
                   help="resize on the device instead of with PIL on the host: the same sizes, the inputs passed as they are "
                        "with pipe(..., work_size=, output_size=, resample=); the image encoder's preprocessing moves to the device too")
    p.add_argument("--resample", choices=["bilinear", "bicubic", "lanczos"], default=None,
                   help="filter of --device_resize (default bilinear, the reference's); refused without --device_resize")
    p.add_argument("--gt_path", type=str, default=None, metavar="DIR",
                   help="score every saved image against the file of the same name in DIR (at the output size): PSNR / SSIM per "
                        "file and on average, written to metrics.json in the output directory (instantir_amd.metrics)")
    p.add_argument("--metrics", choices=["psnr", "ssim"], nargs="+", default=None,
                   help="the figures of --gt_path / --input_fidelity (default: psnr ssim)")
    p.add_argument("--metrics_y", action="store_true", help="score the BT.601 luma channel alone, as super-resolution tables do")
    p.add_argument("--metrics_crop", type=int, default=None, metavar="N", help="drop N border pixels on every side before scoring")
    p.add_argument("--input_fidelity", action="store_true",
                   help="score every saved image, resized to its input's size (bicubic), against the input file as it was read: "
                        "how far the restoration moved from what it was given; needs no ground truth")
    p.add_argument("--lpips_path", type=str, default=None, metavar="PATH",
                   help="add LPIPS (VGG-16) to every pair --gt_path / --input_fidelity score: a whole lpips.LPIPS state dict, or a "
                        "torchvision VGG-16 state dict together with --lpips_lin_path (instantir_amd.lpips)")
    p.add_argument("--lpips_lin_path", type=str, default=None, metavar="PATH",
                   help="the lin layers of LPIPS (lpips' vgg.pth) when --lpips_path is a torchvision VGG-16 state dict")
    p.add_argument("--dists_path", type=str, default=None, metavar="PATH",
                   help="add DISTS (VGG-16) to every pair --gt_path / --input_fidelity score: a whole DISTS state dict, or a "
                        "torchvision VGG-16 state dict together with --dists_weights_path (instantir_amd.dists)")
    p.add_argument("--dists_weights_path", type=str, default=None, metavar="PATH",
                   help="alpha and beta of DISTS (its weights.pt) when --dists_path is a torchvision VGG-16 state dict")
    p.add_argument("--niqe_path", type=str, default=None, metavar="PARAMS",
                   help="score every saved image with NIQE (no ground truth needed) under the pristine model in PARAMS: basicsr's "
                        "niqe_pris_params.npz, the MATLAB release's .mat, or `python -m instantir_amd.niqe fit`'s output; with "
                        "--input_fidelity the input file is scored too (input_niqe); --metrics_crop applies")
    p.add_argument("--degrade", type=str, default=None, metavar="PRESET_OR_JSON",
                   help="the files of --test_path are clean images: degrade each on the device first, with a recipe sampled from "
                        "the preset (realesrgan, bicubic) per (--degrade_seed, file name) or read from a recipe JSON file; the "
                        "8-bit LQ image and its recipe go to lq/ in the output directory, and --gt_path defaults to --test_path")
    p.add_argument("--degrade_seed", type=int, default=None, metavar="N", help="seed of --degrade's recipes and noise (default 0)")
    return p


def apply_degrade(args):
    """`--degrade PRESET_OR_JSON [--degrade_seed N]` -> {"spec", "seed"} or None (an addition: the reference's infer.py reads
    LQ files that something else made).  Refused: the seed without the flag, a negative seed, an unknown preset or an unreadable
    JSON, and a recipe that leaves the LQ at 1 / sf of the size (`resize_lq` false) together with a ground-truth comparison.
    Without `--gt_path` and `--input_fidelity`, `--gt_path` becomes the directory of `--test_path`: the clean files."""
    spec, seed = getattr(args, "degrade", None), getattr(args, "degrade_seed", None)
    if spec is None:
        if seed is not None:
            raise SystemExit("--degrade_seed needs --degrade")
        return None
    seed = 0 if seed is None else seed
    if seed < 0:
        raise SystemExit(f"--degrade_seed must be >= 0, got {seed}")
    from . import degrade as D
    try:
        probe = D.load_recipe(spec, seed, "")
    except ValueError as e:
        raise SystemExit(f"--degrade: {e}")
    if getattr(args, "gt_path", None) is None and not getattr(args, "input_fidelity", False):
        args.gt_path = args.test_path if os.path.isdir(args.test_path) else (os.path.dirname(args.test_path) or ".")
    if not probe.resize_lq and getattr(args, "gt_path", None) is not None:
        raise SystemExit("--degrade: this recipe leaves the LQ at 1 / sf of the clean size (resize_lq false), which cannot be "
                         "scored against --gt_path")
    return {"spec": spec, "seed": int(seed)}


def degraded_input(setup, im, name, out_dir, device):
    """The clean image `im` of file `name` -> its LQ image as the 8-bit PIL image the run goes on with; saved as PNG to
    <out_dir>/lq/<name>, its recipe to <out_dir>/lq/<stem>.json.  One launch chain per file, seeded by (seed, name): a file's LQ
    does not depend on its batch."""
    from . import degrade as D
    recipe = D.load_recipe(setup["spec"], setup["seed"], name)
    lq = Image.fromarray(D.quantize_u8(D.degrade([im], recipe, seed=D.noise_seed(setup["seed"], name), device=device))[0])
    lq_dir = os.path.join(out_dir, "lq")
    os.makedirs(lq_dir, exist_ok=True)
    lq.save(os.path.join(lq_dir, name), format="PNG")
    with open(os.path.join(lq_dir, os.path.splitext(name)[0] + ".json"), "w") as f:
        f.write(recipe.to_json())
    return lq


def apply_metrics(args):
    """`--gt_path DIR` / `--input_fidelity` with `--metrics`, `--metrics_y`, `--metrics_crop` -> the scoring settings, or None
    when nothing is scored (an addition: the reference's infer.py reports no figures).  An option flag without either of the
    two is refused, as is a GT directory that does not exist."""
    gt = getattr(args, "gt_path", None)
    fidelity = bool(getattr(args, "input_fidelity", False))
    names, y, crop = getattr(args, "metrics", None), bool(getattr(args, "metrics_y", False)), getattr(args, "metrics_crop", None)
    if gt is None and not fidelity:
        for flag, on in (("--metrics", names is not None), ("--metrics_y", y), ("--metrics_crop", crop is not None)):
            if on and not (flag == "--metrics_crop" and getattr(args, "niqe_path", None) is not None):
                raise SystemExit(f"{flag} needs --gt_path or --input_fidelity")
        return None
    if crop is not None and crop < 0:
        raise SystemExit(f"--metrics_crop must be >= 0, got {crop}")
    if gt is not None and not os.path.isdir(gt):
        raise SystemExit(f"--gt_path {gt} is not a directory")
    names = tuple(n for n in ("psnr", "ssim") if n in (names or ("psnr", "ssim")))
    return {"gt_path": gt, "input_fidelity": fidelity, "metrics": names, "y_channel": y, "crop_border": int(crop or 0)}


# the pair scorers: name -> (path flag, second-file flag, second-file keyword of the settings, module, class)
PAIR_SCORERS = {"lpips": ("lpips_path", "lpips_lin_path", "lin_path", "lpips", "LPIPS"),
                "dists": ("dists_path", "dists_weights_path", "weights_path", "dists", "DISTS")}


def apply_pair_scorer(name, args):
    """`--lpips_path PATH [--lpips_lin_path PATH]` -> {"path", "lin_path"}, `--dists_path PATH [--dists_weights_path PATH]` ->
    {"path", "weights_path"}, or None without the flag (an addition: the reference builds LPIPS for training only,
    losses/losses.py:81-95, and reports no figures).  Refused: the second file without the flag, the flag without a comparison
    to add the figure to, and a file that does not exist."""
    flag, second_flag, second_key = PAIR_SCORERS[name][:3]
    path, second = getattr(args, flag, None), getattr(args, second_flag, None)
    if path is None:
        if second is not None:
            raise SystemExit(f"--{second_flag} needs --{flag}")
        return None
    if getattr(args, "gt_path", None) is None and not getattr(args, "input_fidelity", False):
        raise SystemExit(f"--{flag} needs --gt_path or --input_fidelity")
    for fl, f in ((flag, path), (second_flag, second)):
        if f is not None and not os.path.isfile(f):
            raise SystemExit(f"--{fl} {f} is not a file")
    return {"path": path, second_key: second}


def apply_niqe(args):
    """`--niqe_path PARAMS` -> {"path", "crop_border", "input"}, or None without the flag (an addition: the reference reports no
    figures).  NIQE needs no comparison: the flag stands on its own, takes `--metrics_crop`, and with `--input_fidelity` scores
    the input file as well.  Refused: a file that does not exist, a negative crop."""
    path = getattr(args, "niqe_path", None)
    if path is None:
        return None
    if not os.path.isfile(path):
        raise SystemExit(f"--niqe_path {path} is not a file")
    crop = getattr(args, "metrics_crop", None)
    if crop is not None and crop < 0:
        raise SystemExit(f"--metrics_crop must be >= 0, got {crop}")
    return {"path": path, "crop_border": int(crop or 0), "input": bool(getattr(args, "input_fidelity", False))}


def build_niqe(setup):
    """The pristine model of `apply_niqe`'s settings; a file that does not hold one ends the run."""
    from .niqe import NIQE
    try:
        return NIQE.from_file(setup["path"])
    except (ValueError, OSError) as e:
        raise SystemExit(f"--niqe_path: {e}")


def score_niqe(setup, model, saved_path, original, device):
    """{"niqe"} of the saved file as it was saved (read back) and, when asked for, {"input_niqe"} of `original`."""
    from . import metrics as M
    row = {}
    try:
        row["niqe"] = M.niqe(Image.open(saved_path).convert("RGB"), model, crop_border=setup["crop_border"], device=device)
        if setup["input"]:
            row["input_niqe"] = M.niqe(original, model, crop_border=setup["crop_border"], device=device)
    except ValueError as e:
        raise SystemExit(f"{saved_path}: {e}")
    return row


def build_pair_scorer(name, setup, device):
    """The model of `apply_pair_scorer`'s settings on `device`; a file that is not one of its two formats ends the run."""
    import importlib
    flag, _, second_key, module, cls = PAIR_SCORERS[name]
    try:
        return getattr(importlib.import_module("." + module, __package__), cls).from_files(setup["path"], setup[second_key], device=device)
    except ValueError as e:
        raise SystemExit(f"--{flag}: {e}")


def gt_image(setup, name, size):
    """The ground truth of input `name` at `size` = (width, height); a missing file or another size ends the run, naming it."""
    path = os.path.join(setup["gt_path"], name)
    if not os.path.isfile(path):
        raise SystemExit(f"--gt_path: {path} does not exist (every input needs a file of its own name)")
    im = Image.open(path).convert("RGB")
    if im.size != tuple(size):
        raise SystemExit(f"--gt_path: {path} is {im.size[0]}x{im.size[1]} but the output is {size[0]}x{size[1]}")
    return im


def score_saved(setup, saved_path, gt, original, device, models=None):
    """The figures of one saved file, from the 8-bit image as it was saved (read back): {"psnr", "ssim"} against `gt`,
    {"input_psnr", "input_ssim"} against `original`, whichever were asked for; with `models` {"lpips": model} "lpips" /
    "input_lpips" too, with {"dists": model} "dists" / "input_dists"."""
    from . import metrics as M
    saved = Image.open(saved_path).convert("RGB")
    kw = dict(metrics=setup["metrics"], crop_border=setup["crop_border"], y_channel=setup["y_channel"], device=device)
    kw.update({name + "_model": model for name, model in (models or {}).items()})
    row = {}
    try:
        if gt is not None:
            row.update({k: v[0] for k, v in M.evaluate(saved, gt, **kw).items() if not k.endswith("_mean")})
        if original is not None:
            row.update({"input_" + k: v[0] for k, v in M.input_fidelity(saved, original, **kw).items() if not k.endswith("_mean")})
    except ValueError as e:
        raise SystemExit(f"{saved_path}: {e}")
    return row


def write_metrics(setup, rows, out_dir, rank=0, world=1):
    """metrics.json (metrics.rank{r}.json with more than one rank): the settings, the per-file figures and their means; returns
    the summary line."""
    import json
    keys = sorted({k for row in rows.values() for k in row})
    mean = {k: float(sum(row[k] for row in rows.values()) / len(rows)) for k in keys} if rows else {}
    path = os.path.join(out_dir, "metrics.json" if world == 1 else f"metrics.rank{rank}.json")
    with open(path, "w") as f:
        json.dump({"settings": setup, "files": rows, "mean": mean}, f, indent=1, sort_keys=True)
    return f"metrics over {len(rows)} file(s): " + ", ".join(f"{k} {mean[k]:.4f}" for k in keys) + f" -> {path}"


def apply_device_resize(pipe, args):
    """`--device_resize [--resample F]` -> whether the call resizes on the device, and its filter (an addition: the reference
    resizes with PIL twice).  `--resample` without `--device_resize` is refused; `pipe` None only checks the flags."""
    on = bool(getattr(args, "device_resize", False))
    flt = getattr(args, "resample", None)
    if flt is not None and not on:
        raise SystemExit("--resample needs --device_resize (the host path resizes with PIL's bilinear filter, as the reference does)")
    if on and pipe is not None:
        pipe.enable_device_preprocess()
    return on, flt or "bilinear"


def build_pipeline(args, device):
    """infer.py:117-144 against this build's classes."""
    from . import loaders, weights as W
    from .config import UNetConfig, VAEConfig
    from .encoders import HipCLIPText, HipDinov2
    from .pipeline import InstantIRPipeline
    from .schedulers import DDPMScheduler, LCMSingleStepScheduler
    from .vae import HipVAE
    if args.synthetic:
        cfg = UNetConfig.tiny() if args.synthetic == "tiny" else UNetConfig.sdxl()
        vc = VAEConfig.tiny() if args.synthetic == "tiny" else VAEConfig.sdxl()
        gen = "cpu" if args.synthetic == "tiny" else device
        unet_sd = W.synth_state_dict(W.unet_specs(cfg), 1234, device=gen)
        agg_sd = W.synth_state_dict(W.aggregator_specs(cfg), 1235, device=gen)
        lora, alpha = W.synth_state_dict(W.lora_specs(cfg), 1236, device=gen), max(1, cfg.lora_rank // 8)
        vae = HipVAE(vc, W.synth_state_dict(W.vae_decoder_specs(vc) + W.vae_encoder_specs(vc), 1237, device=gen), device)
        pipe = InstantIRPipeline(cfg, unet_sd, scheduler=DDPMScheduler(), vae=vae, device=device)
        pipe.prepare_previewers(lora, lora_alpha=alpha)
        pipe.aggregator.load_state_dict(agg_sd)
        return pipe, LCMSingleStepScheduler.from_config(pipe.scheduler.config)
    if not args.sdxl_path or not args.instantir_path:
        raise SystemExit("--sdxl_path and --instantir_path are required (or use --synthetic)")
    # infer.py:117-144, call for call
    print("Initializing pipeline...")
    pipe = InstantIRPipeline.from_pretrained(args.sdxl_path, torch_dtype=torch.float16, device=device)
    print("Loading LQ-Adapter...")
    adapter = args.adapter_model_path if args.adapter_model_path is not None else os.path.join(args.instantir_path, "adapter.pt")
    # (the reference parses --adapter_tokens but never forwards it, infer.py:124-129,269; forwarded here: default 64 is the same call)
    loaders.load_adapter_to_pipe(pipe, adapter, args.vision_encoder_path, use_clip_encoder=args.use_clip_encoder,
                                 adapter_tokens=args.adapter_tokens)
    lora_path = args.previewer_lora_path if args.previewer_lora_path is not None else args.instantir_path
    lora_alpha = pipe.prepare_previewers(lora_path)
    print(f"use lora alpha {lora_alpha}")
    pipe.scheduler = DDPMScheduler.from_pretrained(args.sdxl_path, subfolder="scheduler") \
        if os.path.isfile(os.path.join(args.sdxl_path, "scheduler", "scheduler_config.json")) else DDPMScheduler()
    lcm_scheduler = LCMSingleStepScheduler.from_config(pipe.scheduler.config)
    print("Loading checkpoint...")
    pipe.aggregator.load_state_dict(loaders.read_aggregator(os.path.join(args.instantir_path, "aggregator.pt")))
    return pipe, lcm_scheduler


def apply_scheduler(pipe, args):
    """`--scheduler NAME [--karras]` -> pipe.scheduler = Cls.from_config(pipe.scheduler.config, ...) (an addition: the
    reference's infer.py always runs DDPMScheduler).  The default, ddpm without --karras, leaves the pipeline as built."""
    from . import schedulers as S
    name = getattr(args, "scheduler", "ddpm") or "ddpm"
    karras = bool(getattr(args, "karras", False))
    if karras and name not in ("euler", "dpmpp_2m", "dpmpp_2m_sde"):
        raise SystemExit(f"--karras applies to euler, dpmpp_2m and dpmpp_2m_sde, not to {name}")
    if name == "ddpm":
        return
    cls_name, kw = SCHEDULERS[name]
    kw = dict(kw)
    if karras:
        kw["use_karras_sigmas"] = True
    pipe.scheduler = getattr(S, cls_name).from_config(pipe.scheduler.config, **kw)


def apply_freeu(pipe, args):
    """`--freeu S1 S2 B1 B2` -> pipe.enable_freeu(...) (an addition: the reference's infer.py has no such flag; its pipeline has
    the switch).  Without the flag the pipeline is left as built (FreeU off)."""
    if getattr(args, "freeu", None) is not None:
        pipe.enable_freeu(*args.freeu)


def apply_seg(pipe, args):
    """`--seg_scale S` (> 0) -> pipe.enable_seg(--seg_layers split at commas, --seg_blur_sigma); returns the call's SEG keyword
    arguments (an addition: the reference has no SEG).  With `--pag_scale` as well, enable_seg refuses (ValueError)."""
    scale = float(getattr(args, "seg_scale", 0.0) or 0.0)
    if scale < 0:
        raise SystemExit(f"--seg_scale must be >= 0, got {scale}")
    if scale == 0:
        return {}
    layers = [e.strip() for e in str(getattr(args, "seg_layers", "mid") or "").split(",") if e.strip()]
    pipe.enable_seg(layers, getattr(args, "seg_blur_sigma", 100.0))
    return {"seg_scale": scale}


def apply_pag(pipe, args):
    """`--pag_scale S` (> 0) -> pipe.enable_pag(--pag_layers split at commas); returns the call's PAG keyword arguments (an
    addition: the reference has no PAG).  `--pag_adaptive_scale` without `--pag_scale` is refused."""
    scale = float(getattr(args, "pag_scale", 0.0) or 0.0)
    adaptive = float(getattr(args, "pag_adaptive_scale", 0.0) or 0.0)
    if scale < 0:
        raise SystemExit(f"--pag_scale must be >= 0, got {scale}")
    if scale == 0:
        if adaptive:
            raise SystemExit("--pag_adaptive_scale needs --pag_scale > 0")
        return {}
    layers = [e.strip() for e in str(getattr(args, "pag_layers", "mid") or "").split(",") if e.strip()]
    pipe.enable_pag(layers)
    return {"pag_scale": scale, "pag_adaptive_scale": adaptive}


def apply_apg(pipe, args):
    """`--apg ETA NORM_THRESHOLD MOMENTUM` -> pipe.enable_apg(...) (an addition: the reference has no APG).  Without the flag the
    pipeline is left as built (APG off)."""
    if getattr(args, "apg", None) is not None:
        pipe.enable_apg(*args.apg)


def apply_vae_flash_attention(pipe, args):
    """`--vae_flash_attention` -> pipe.vae.enable_flash_attention() (an addition: the reference's VAE attention goes through
    torch SDPA at any size).  Without the flag the VAE is left as built (three GEMMs around a row softmax, 16384-pixel ceiling)."""
    if getattr(args, "vae_flash_attention", False):
        if pipe.vae is None:
            raise SystemExit("--vae_flash_attention needs a pipeline with a VAE")
        pipe.vae.enable_flash_attention()


def apply_color_fix(args):
    """`--color_fix {none,wavelet,adain}` -> the call's `color_fix` keyword argument (an addition: the reference has no colour
    fix).  `none`, the default, adds nothing to the call."""
    mode = getattr(args, "color_fix", "none") or "none"
    if mode not in ("none", "wavelet", "adain"):
        raise SystemExit(f"--color_fix must be none, wavelet or adain, got {mode}")
    return {} if mode == "none" else {"color_fix": mode}


def apply_restore_map(args, names, size):
    """`--restore_map PATH [--map_feather N]` -> the call's `restore_map` / `map_feather` keyword arguments for the inputs
    `names`, each map resized to `size` = (width, height) of the resized inputs with Image.BILINEAR (an addition: the reference
    has no regional control).  PATH is one file for every input or a directory with a map per input file name; an input
    without a map is an error naming it.  Without the flag nothing is added to the call."""
    path = getattr(args, "restore_map", None)
    feather = getattr(args, "map_feather", 4)
    if feather is None or feather < 0:
        raise SystemExit(f"--map_feather must be >= 0, got {feather}")
    if path is None:
        return {}
    from .restore_map import load_maps
    try:
        return {"restore_map": load_maps(path, names, size), "map_feather": int(feather)}
    except FileNotFoundError as e:
        raise SystemExit(str(e))


def main(args, device, rank=0, world=1):
    apply_device_resize(None, args)              # (a flag error should not wait for the weights to load)
    degrading = apply_degrade(args)              # (before apply_metrics: it may set --gt_path)
    scoring = apply_metrics(args)
    pair_setups = {name: apply_pair_scorer(name, args) for name in PAIR_SCORERS}
    pair_setups = {name: s for name, s in pair_setups.items() if s}
    niqe_setup = apply_niqe(args)
    niqe_model = build_niqe(niqe_setup) if niqe_setup else None
    pipe, lcm_scheduler = build_pipeline(args, device)
    pair_models = {name: build_pair_scorer(name, s, device) for name, s in pair_setups.items()}
    apply_freeu(pipe, args)
    apply_scheduler(pipe, args)
    pag_kw = apply_pag(pipe, args)
    pag_kw.update(apply_seg(pipe, args))
    apply_apg(pipe, args)
    pag_kw.update(apply_color_fix(args))
    apply_vae_flash_attention(pipe, args)
    device_resize, resample = apply_device_resize(pipe, args)
    post_fix = f"_{args.post_fix}" if args.post_fix else ""
    out_dir = f"{args.out_path}/{post_fix}"
    os.makedirs(out_dir, exist_ok=True)
    cfg = pipe.cfg
    batches = plan_batches(args.test_path, os.path.join(args.out_path, post_fix), args.batch_size)
    scores = {}
    for lq_batch in shard_batches(batches, rank, world):
        generator = torch.Generator(device=device).manual_seed(args.seed)                # infer.py:172: fresh per batch
        lq, out_sizes, work_sizes, originals = [], [], [], []
        for name in lq_batch:
            path = args.test_path if os.path.isfile(args.test_path) else os.path.join(args.test_path, name)
            im = Image.open(path).convert("RGB")
            if degrading:
                im = degraded_input(degrading, im, name, out_dir, device)
            originals.append(im)
            if device_resize:
                work, out_size = resize_plan(im.size, width=args.width, height=args.height)
                work_sizes.append(work)
            else:
                im, out_size = resize_img(im, width=args.width, height=args.height)
            lq.append(im)
            out_sizes.append(out_size)
        if len({im.size for im in lq}) != 1:
            raise ValueError("images of one batch must share a size after resize_img (use --width/--height or --batch_size 1)")
        if device_resize and len(set(out_sizes)) != 1:
            raise ValueError("images of one batch must share an output size with --device_resize (use --batch_size 1)")
        work_w, work_h = work_sizes[0] if device_resize else lq[0].size
        gts = [gt_image(scoring, n, s) for n, s in zip(lq_batch, out_sizes)] if scoring and scoring["gt_path"] else None
        # infer.py:191-210: `--prompt` / `--neg_prompt` are nargs="*" LISTS and the reference multiplies the list by the batch
        # (`prompt = args.prompt * len(lq)`): `--prompt "a photo" "a drawing"` with one image asks for two restorations, one per
        # entry; with several images AND several entries the pipeline's own batch check (:1316-1319) rejects the call.
        prompts = (list(args.prompt) if args.prompt else [DEFAULT_PROMPT]) * len(lq)
        negs = (list(args.neg_prompt) if args.neg_prompt else [DEFAULT_NEG_PROMPT]) * len(lq)
        kw = dict(image=lq, num_inference_steps=args.num_inference_steps, generator=generator, guidance_scale=args.cfg,
                  previewer_scheduler=lcm_scheduler, preview_start=args.preview_start, control_guidance_end=args.creative_start,
                  **pag_kw, **apply_restore_map(args, lq_batch, (work_w, work_h)))
        if device_resize:
            kw.update(work_size=(work_h, work_w), output_size=(out_sizes[0][1], out_sizes[0][0]), resample=resample)
        if args.synthetic:
            g = torch.Generator().manual_seed(args.seed)
            n = len(lq)
            kw.update(prompt_embeds=torch.randn(n, cfg.text_len, cfg.cross_attention_dim, generator=g),
                      pooled_prompt_embeds=torch.randn(n, cfg.pooled_dim, generator=g),
                      negative_prompt_embeds=torch.randn(n, cfg.text_len, cfg.cross_attention_dim, generator=g),
                      negative_pooled_prompt_embeds=torch.randn(n, cfg.pooled_dim, generator=g),
                      ip_adapter_image_embeds=[torch.randn(2 if args.cfg > 1 else 1, n, cfg.resampler.seq_len, cfg.resampler.embedding_dim, generator=g)])
        else:
            kw.update(prompt=prompts, negative_prompt=negs)
            if not device_resize:          # (on the device the default stands in: the working image, preprocessed there)
                kw.update(ip_adapter_image=lq)
        images = pipe(**kw).images
        for i, (rec, out_size) in enumerate(zip(images, out_sizes)):
            if not device_resize:
                rec = rec.resize([out_size[0], out_size[1]], Image.BILINEAR)
            rec.save(f"{out_dir}/{lq_batch[i]}")
            if scoring:
                scores[lq_batch[i]] = score_saved(scoring, f"{out_dir}/{lq_batch[i]}", gts[i] if gts else None,
                                                  originals[i] if scoring["input_fidelity"] else None, device, pair_models)
            if niqe_setup:
                scores.setdefault(lq_batch[i], {}).update(score_niqe(niqe_setup, niqe_model, f"{out_dir}/{lq_batch[i]}", originals[i], device))
    if scoring or niqe_setup:
        setup = dict(scoring or {}, **pair_setups)
        if niqe_setup:
            setup["niqe"] = niqe_setup
        print(write_metrics(setup, scores, out_dir, rank, world))


if __name__ == "__main__":
    a = build_parser().parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("instantir_amd.infer needs an MI355X: the restoration path has no CPU fallback")
    # one process per GPU: `python -m torch.distributed.run --nproc-per-node N -m instantir_amd.infer ...` shards the inputs
    from .parallel import barrier, init_from_env
    rank_, world_, _, dev_ = init_from_env()
    main(a, dev_, rank_, world_)
    if world_ > 1:
        barrier()
        torch.distributed.destroy_process_group()
