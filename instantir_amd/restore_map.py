"""Host side of region-selective restoration (`restore_map=` of InstantIRPipeline.__call__; DESIGN.md section 7 "Restore map").

A restore map holds one value s in [0, 1] per pixel: the fraction of the schedule, counted from its end, during which the
pixel is denoised freely.  s = 1 is free in every step (the behaviour without a map), s = 0 is never free (the pixel comes
out as the LQ input), s = 0.3 is free for the last 30 % of the steps.  Everything here is plain host arithmetic and tensor
plumbing: the per-step threshold and noise pair the step kernel reads, the checks on a caller's map, and the CLI's lookup of
map files."""
from __future__ import annotations

import os

import numpy as np
import torch


def thresholds(n_steps):
    """thr_i = (N - 1 - i) / N for the N steps the loop runs: a pixel with map value s is KEPT in step i when s <= thr_i
    (compared in fp32).  The last step's threshold is 0 (only s = 0 is still kept), and every threshold is below 1 (s = 1 is
    never kept)."""
    n = int(n_steps)
    if n < 1:
        raise ValueError(f"a restore map needs at least one step, got {n_steps}")
    return [(n - 1 - i) / n for i in range(n)]


def free_steps(s, n_steps):
    """Number of steps in which a pixel of map value `s` is denoised freely (the fp32 compare the kernel makes)."""
    s32 = np.float32(s)
    return sum(1 for thr in thresholds(n_steps) if not s32 <= np.float32(thr))


def keep_pair(scheduler, i, t):
    """(a, b) of keep = a * lq + b * noise0 after loop step i at timestep t: the pair `scheduler.add_noise` uses for the
    timetable entry that FOLLOWS the step, (1, 0) when the step is the scheduler's last entry."""
    if hasattr(scheduler, "_noise_pair"):                       # sigma schedulers: the loop index is the scheduler's
        if i + 1 >= len(scheduler.timesteps):
            return 1.0, 0.0
        a, b = scheduler._noise_pair(i + 1)
        return float(a), float(b)
    ts = [int(v) for v in scheduler.timesteps]
    idx = ts.index(int(t))
    if idx + 1 >= len(ts):
        return 1.0, 0.0
    tn = torch.tensor([ts[idx + 1]])
    acp = scheduler.alphas_cumprod                              # the expressions of _Base.add_noise, on the fp32 table
    return float((acp[tn] ** 0.5)[0]), float(((1 - acp[tn]) ** 0.5)[0])


def check_feather(map_feather):
    from .ops import MAX_MAP_FEATHER
    if isinstance(map_feather, bool) or int(map_feather) != map_feather or map_feather < 0:
        raise ValueError(f"map_feather must be a non-negative integer (pixels), got {map_feather!r}")
    if map_feather > MAX_MAP_FEATHER:
        raise ValueError(f"map_feather must be at most {MAX_MAP_FEATHER} pixels, got {map_feather}")
    return int(map_feather)


def as_tensor(restore_map):
    """A caller's map as an fp32 tensor (n, 1, H, W) on the device it came on: PIL image(s) (converted to "L", / 255), a
    tensor or an array of shape (H, W) or (n, 1, H, W)."""
    if isinstance(restore_map, (list, tuple)) and restore_map and all(hasattr(m, "convert") for m in restore_map):
        if len({m.size for m in restore_map}) != 1:
            raise ValueError("restore_map: the PIL maps of one call must share a size")
        return torch.stack([as_tensor(m)[0] for m in restore_map])
    if hasattr(restore_map, "convert"):
        a = np.asarray(restore_map.convert("L"), dtype=np.float32) / 255.0
        return torch.from_numpy(a)[None, None]
    if isinstance(restore_map, np.ndarray):
        restore_map = torch.from_numpy(restore_map)
    if not torch.is_tensor(restore_map):
        raise ValueError(f"restore_map must be a PIL image, a list of them, a tensor or an array, got {type(restore_map).__name__}")
    m = restore_map
    if m.dim() == 2:
        m = m[None, None]
    if m.dim() != 4 or m.shape[1] != 1:
        raise ValueError(f"restore_map has shape {tuple(restore_map.shape)}, expected (H, W) or (n, 1, H, W)")
    return m.to(torch.float32)


def prepare(restore_map, B, nipp, pixel_size, latent_size, device):
    """Checks a caller's map and expands it over the batch as `lq` is (one map serves the whole batch, otherwise each map is
    repeated per `num_images_per_prompt` copy) -> (map (B, H, W) fp32 contiguous on `device`, whether it is at pixel size).
    `pixel_size` / `latent_size`: the two (H, W) a map may have."""
    m = as_tensor(restore_map)
    if not bool(torch.isfinite(m).all()):
        raise ValueError("restore_map holds non-finite values; it must lie in [0, 1]")
    lo, hi = float(m.min()), float(m.max())
    if lo < 0.0 or hi > 1.0:
        raise ValueError(f"restore_map values must lie in [0, 1], got [{lo}, {hi}]")
    size = tuple(m.shape[2:])
    if size == tuple(pixel_size):
        at_pixels = True
    elif size == tuple(latent_size):
        at_pixels = False
    else:
        raise ValueError(f"restore_map has size {size}: it must match the image {tuple(pixel_size)} or the latent {tuple(latent_size)}")
    m = m.repeat(B, 1, 1, 1) if m.shape[0] == 1 else m.repeat_interleave(nipp, 0)
    if m.shape[0] != B:
        raise ValueError(f"restore_map gives {m.shape[0]} maps, the batch has {B}")
    return m[:, 0].to(device, torch.float32).contiguous(), at_pixels


# ---- the CLI's `--restore_map PATH` -------------------------------------------------------------------------------
def map_path_for(restore_map, name):
    """The map file of input `name`: `restore_map` itself when it is a file (one map for every input), otherwise the entry of
    the directory with the input's file name, or with its stem and any extension."""
    if os.path.isfile(restore_map):
        return restore_map
    if not os.path.isdir(restore_map):
        raise FileNotFoundError(f"--restore_map {restore_map}: no such file or directory")
    exact = os.path.join(restore_map, name)
    if os.path.isfile(exact):
        return exact
    stem = os.path.splitext(name)[0]
    for f in sorted(os.listdir(restore_map)):
        if os.path.splitext(f)[0] == stem and os.path.isfile(os.path.join(restore_map, f)):
            return os.path.join(restore_map, f)
    raise FileNotFoundError(f"--restore_map {restore_map}: no map for input {name}")


def load_maps(restore_map, names, size):
    """One "L" PIL map per input name, resized to `size` = (width, height) of the resized inputs with Image.BILINEAR."""
    from PIL import Image
    return [Image.open(map_path_for(restore_map, n)).convert("L").resize(list(size), Image.BILINEAR) for n in names]
