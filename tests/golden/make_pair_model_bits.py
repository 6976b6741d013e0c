"""Bits of the two VGG-16 pair scorers, recorded through instantir_amd.lpips.LPIPS, instantir_amd.dists.DISTS and metrics.

    python tests/golden/make_pair_model_bits.py          # on an MI355X: writes tests/golden/pair_model_bits.npz

`replay()` scores seeded pairs with seeded stand-in networks and returns every output whole, as an integer view.  The committed
file was written by the tree as it stood before LPIPS and DISTS shared instantir_amd/vgg.py (two recordings, equal);
tests/test_pair_model_bits_gpu.py replays on the current tree and asserts equality, so a launch that moved, a view of another
buffer or a changed halving shows where the fp64 restatements' tolerances could hide it.

The cases:
  models    LPIPS.synthetic and DISTS.synthetic, fp16 and bf16, widths (8, 16, 16, 24, 8), 17 x 19 (floor and ceil halving part
            ways at every level), N = 2: one uint8 pair, one fp32 pair and, for DISTS, one mixed uint8 / fp32 pair.  LPIPS with
            layers=True, spatial=True (the (N, 5) terms and all five maps), DISTS with components=True.
  wide      widths (72, 136, 64, 8, 264), whose padding differs per stage, fp16, 33 x 18, N = 1, both classes.
  metrics   metrics.evaluate (17 x 19) and metrics.input_fidelity with both models given: the result's keys in order and its
            values as float bits.  input_fidelity scores a 35 x 37 restoration against a 17 x 19 `lq`; against a 9 x 10 `lq`
            it refuses (the SSIM window needs 11 pixels, both networks 16), and the refusal's text is the recorded result.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "pair_model_bits.npz")

NARROW, WIDE = (8, 16, 16, 24, 8), (72, 136, 64, 8, 264)


def _bits(t):
    a = t.detach().cpu().contiguous().numpy()
    return a.view({1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize])


def _pair(seed, N, H, W):
    """(a, b) as uint8 (N, H, W, 3) and as fp32 (N, 3, H, W) off the 8-bit grid: b is a within +-20 levels."""
    rng = np.random.RandomState(seed)
    a8 = rng.randint(0, 256, (N, H, W, 3)).astype(np.uint8)
    b8 = np.clip(a8.astype(np.int32) + rng.randint(-20, 21, a8.shape), 0, 255).astype(np.uint8)
    af = np.clip(a8.transpose(0, 3, 1, 2) / 255.0 + rng.uniform(-0.002, 0.002, (N, 3, H, W)), 0.0, 1.0).astype(np.float32)
    bf = np.clip(b8.transpose(0, 3, 1, 2) / 255.0 + rng.uniform(-0.002, 0.002, (N, 3, H, W)), 0.0, 1.0).astype(np.float32)
    return a8, b8, af, bf


def _result(out, key, res):
    """A metrics result (or the text of its refusal) into `out`: the keys in order, the values as float bits."""
    if isinstance(res, str):
        out[key + ".refused"] = np.array(res)
        return
    out[key + ".keys"] = np.array(list(res))
    for k, v in res.items():
        out[f"{key}.{k}"] = np.atleast_1d(np.asarray(v, dtype=np.float64)).view(np.int64)


def replay():
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from instantir_amd import metrics as M
    from instantir_amd.dists import DISTS
    from instantir_amd.lpips import LPIPS
    dev = torch.device("cuda:0")
    t = torch.from_numpy
    out = {}

    def lpips(key, model, a, b):
        score, maps = model(a, b, layers=True, spatial=True)
        out[key + ".layers"] = _bits(score)
        for l, m in enumerate(maps):
            out[f"{key}.map{l}"] = _bits(m)

    def dists(key, model, a, b):
        score, terms = model(a, b, components=True)
        out[key + ".score"], out[key + ".terms"] = _bits(score), _bits(terms)

    a8, b8, af, bf = _pair(20250, 2, 17, 19)
    for dtype in (torch.float16, torch.bfloat16):
        name = str(dtype).split(".")[1]
        lp, ds = LPIPS.synthetic(7, NARROW, device=dev, dtype=dtype), DISTS.synthetic(9, NARROW, device=dev, dtype=dtype)
        lpips(f"lpips.{name}.u8", lp, a8, b8)
        lpips(f"lpips.{name}.f32", lp, t(af), t(bf))
        dists(f"dists.{name}.u8", ds, a8, b8)
        dists(f"dists.{name}.f32", ds, t(af), t(bf))
        dists(f"dists.{name}.mixed", ds, a8, t(bf))

    w8a, w8b, _, _ = _pair(20251, 1, 33, 18)
    lpips("lpips.wide", LPIPS.synthetic(11, WIDE, device=dev), w8a, w8b)
    dists("dists.wide", DISTS.synthetic(13, WIDE, device=dev), w8a, w8b)

    lp, ds = LPIPS.synthetic(7, NARROW, device=dev), DISTS.synthetic(9, NARROW, device=dev)
    _result(out, "evaluate", M.evaluate(a8, b8, lpips_model=lp, dists_model=ds))
    r8, _, _, _ = _pair(20252, 2, 35, 37)
    _result(out, "input_fidelity", M.input_fidelity(r8, a8, lpips_model=lp, dists_model=ds))
    try:
        small = M.input_fidelity(a8, _pair(20253, 2, 9, 10)[0], lpips_model=lp, dists_model=ds)
    except ValueError as e:
        small = str(e)
    _result(out, "input_fidelity.9x10", small)
    torch.cuda.synchronize()
    return out


if __name__ == "__main__":
    path = sys.argv[1] if sys.argv[1:] else PATH
    bits = replay()
    np.savez_compressed(path, **bits)
    print(f"wrote {path}: {len(bits)} buffers, {os.path.getsize(path)} bytes")
