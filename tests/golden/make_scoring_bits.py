"""Bits of the image-scoring and resampling kernels, recorded through instantir_amd.ops.

    python tests/golden/make_scoring_bits.py          # on an MI355X: writes tests/golden/scoring_bits.npz

`replay()` drives ops.image_metrics, ops.niqe_stats, ops.lpips_prep, ops.lpips_tap and ops.resample on seeded inputs and
returns every output whole, as an integer view (a NaN column is compared as its bits).  The committed file was written by the
library as it stood before metrics.hip, niqe.hip, lpips.hip and resample.hip took their pixel read, rounding, luma and
reductions from csrc/image_common.h; tests/test_scoring_bits_gpu.py replays the calls on the current library and asserts
equality, so a reordered sum or a regrouped floating-point statement shows where the fp64 restatements' tolerances hide it.

The shapes are the smallest at which each kernel can still go wrong:
  image_metrics  75 x 70, crop 4: the 57 x 52 SSIM map is 2 x 2 tiles of 32 whose last tiles are partial in both axes and own
                 the 10 trailing pixels; as the MSE alone it is 12462 elements, 7 workgroups, the last one partial.
                 43 x 44, crop 0, one channel: last tiles 1 and 2 map pixels wide.  8 x 8, crop 3: one workgroup, 4 live elements.
  niqe_stats     200 x 300, crop 3: 2 x 3 blocks and pixels beyond the block grid.  96 x 192: the minimum of two blocks; the
                 grid fills the image, so the replicate clamp acts on every edge at both scales.
  lpips_prep     5 x 7 pixels, both source layouts into both 16-bit types, in a view wider than the channel pad.
  lpips_tap      5 x 7: both axes end in an odd remainder quad; one channel count per lane-group width that lpips.hip's
                 dispatch instantiates (1, 2, 4, ..., 64 lanes: the smallest C that selects each), both 16-bit types, negative
                 inputs (the ReLU is in the kernel), `pooled`, `dmap` and `out` all requested.
  resample       uint8 13 x 17 -> 7 x 9 bicubic with quantize; fp32 13 x 17 -> 20 x 11 Lanczos with clamp, scale and bias.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "scoring_bits.npz")

TAP_CHANNELS = (8, 16, 24, 40, 72, 136, 264)          # LP = 1, 2, 4, 8, 16, 32, 64: the smallest C with 8 * LP / 2 < C
FILL = 7.0


def _bits(t):
    a = t.detach().cpu().contiguous().numpy()
    return a.view({1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize])


def replay():
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from instantir_amd import ops
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    out = {}

    # image_metrics
    rng = np.random.RandomState(20240)
    N, H, W = 2, 75, 70
    a8 = rng.randint(0, 256, (N, H, W, 3)).astype(np.uint8)
    b8 = np.clip(a8.astype(np.int32) + rng.randint(-20, 21, a8.shape), 0, 255).astype(np.uint8)
    # fp32 off the 8-bit grid and a little outside [0, 1]: the quantised read rounds and clamps
    af = (a8.transpose(0, 3, 1, 2) / 255.0 + rng.uniform(-0.03, 0.03, (N, 3, H, W))).astype(np.float32)
    c_a = rng.uniform(0, 1, (N, 1, 43, 44)).astype(np.float32)
    c_b = (c_a + rng.standard_normal(c_a.shape) * 0.05).astype(np.float32)
    e_a = rng.randint(0, 256, (N, 8, 8, 1)).astype(np.uint8)
    e_b = rng.randint(0, 256, (N, 8, 8, 1)).astype(np.uint8)
    out["metrics.a"] = _bits(ops.image_metrics(up(a8), up(b8), crop_border=4))
    out["metrics.b"] = _bits(ops.image_metrics(up(af), up(b8), crop_border=4, y_channel=True, quantize=(True, False)))
    out["metrics.c"] = _bits(ops.image_metrics(up(c_a), up(c_b)))
    out["metrics.d"] = _bits(ops.image_metrics(up(a8), up(b8), crop_border=4, what="psnr"))
    out["metrics.e"] = _bits(ops.image_metrics(up(e_a), up(e_b), crop_border=3, what="psnr"))

    # niqe_stats
    rng = np.random.RandomState(20241)
    smooth = lambda shape: np.cumsum(np.cumsum(rng.standard_normal(shape), axis=-2), axis=-1)          # texture with structure
    n_a = smooth((2, 3, 200, 300))
    n_a = (255 * (n_a - n_a.min()) / (n_a.max() - n_a.min())).transpose(0, 2, 3, 1)
    n_a = np.clip(n_a + rng.randint(-12, 13, n_a.shape), 0, 255).astype(np.uint8)
    n_b = smooth((1, 1, 96, 192))
    n_b = ((n_b - n_b.min()) / (n_b.max() - n_b.min()) + rng.uniform(-0.04, 0.04, n_b.shape)).astype(np.float32)
    out["niqe.a"] = _bits(ops.niqe_stats(up(n_a), crop_border=3))
    out["niqe.b"] = _bits(ops.niqe_stats(up(n_b)))

    # lpips_prep
    rng = np.random.RandomState(20242)
    p8 = rng.randint(0, 256, (2, 5, 7, 3)).astype(np.uint8)
    pf = rng.uniform(0, 1, (2, 3, 5, 7)).astype(np.float32)
    for name, src in (("u8", p8), ("f32", pf)):
        for dtype in (torch.float16, torch.bfloat16):
            buf = torch.full((2 * 5 * 7, ops.LPIPS_CPAD + 8), FILL, dtype=dtype, device=dev)
            ops.lpips_prep(up(src), buf[:, :ops.LPIPS_CPAD])
            out[f"lpips_prep.{name}.{str(dtype).split('.')[1]}"] = _bits(buf.view(torch.int16))

    # lpips_tap
    pairs, H, W = 2, 5, 7
    for Cc in TAP_CHANNELS:
        rng = np.random.RandomState(20243 + Cc)
        x = rng.standard_normal((2 * pairs * H * W, Cc)).astype(np.float32)
        lin_w = up(rng.uniform(0, 1, Cc).astype(np.float32))
        for dtype in (torch.float16, torch.bfloat16):
            key = f"lpips_tap.c{Cc}.{str(dtype).split('.')[1]}"
            pooled = torch.full((2 * pairs * (H // 2) * (W // 2), Cc), FILL, dtype=dtype, device=dev)
            dmap = torch.full((pairs, H, W), FILL, dtype=torch.float32, device=dev)
            got = torch.full((pairs,), FILL, dtype=torch.float64, device=dev)
            ops.lpips_tap(up(x).to(dtype), pairs, H, W, lin_w, pooled=pooled, dmap=dmap, out=got)
            out[key + ".pooled"] = _bits(pooled.view(torch.int16))
            out[key + ".dmap"] = _bits(dmap)
            out[key + ".out"] = _bits(got)

    # resample
    rng = np.random.RandomState(20244)
    r8 = rng.randint(0, 256, (2, 13, 17, 3)).astype(np.uint8)
    rf = rng.uniform(-0.2, 1.2, (1, 3, 13, 17)).astype(np.float32)
    out["resample.a"] = _bits(ops.resample(up(r8), (7, 9), filter="bicubic", quantize=True))
    out["resample.b"] = _bits(ops.resample(up(rf), (20, 11), filter="lanczos", clamp=(0.0, 1.0), scale=(2.0, 1.7, 0.9),
                                           bias=(-1.0, 0.25, 0.5)))
    torch.cuda.synchronize()
    return out


if __name__ == "__main__":
    path = sys.argv[1] if sys.argv[1:] else PATH
    bits = replay()
    np.savez_compressed(path, **bits)
    print(f"wrote {path}: {len(bits)} buffers, {os.path.getsize(path)} bytes")
