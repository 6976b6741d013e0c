"""The three degradation launches (ops.filter2d, ops.add_gaussian_noise, ops.jpeg_roundtrip) on one MI355X, beside the torch
compositions they replace.

    python tools/degrade_bench.py [--iters 50] [--windows 5]

One 3-channel fp32 image at 1024^2 and at 2048^2.  Every leg is timed by device events, warm, as the median of `--windows`
windows of `--iters` calls, the windows of all legs alternating.  Each launch stands beside three things measured in the same
run: its byte floor (the image read once and written once, over 6.29 TB/s), an empty call through the same wrapper (the
smallest legal image: the same launch with one workgroup), and the torch composition a user without the entry would write:
F.pad(reflect) + grouped conv2d for the blur, randn + clamp for the noise (another generator: the cost, not the values), and
colour matrices + avg_pool2d + an einsum DCT round trip + nearest upsampling for the JPEG."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

HBM_TBS = 6.29
SIDES = (1024, 2048)


def timed(fn, n):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def torch_filter2d(x, taps):
    N, C, H, W = x.shape
    k = taps.shape[-1]
    p = F.pad(x, (k // 2,) * 4, mode="reflect")
    w = taps.view(N, 1, k, k).repeat_interleave(C, 0)
    return F.conv2d(p.view(1, N * C, *p.shape[-2:]), w, groups=N * C).view(N, C, H, W)


def torch_jpeg(x, q, D, T):
    N, _, H, W = x.shape
    f = (5000.0 / q if q < 50 else 200.0 - 2.0 * q) / 100.0
    fwd = x.new_tensor([[0.299, 0.587, 0.114], [-0.168736, -0.331264, 0.5], [0.5, -0.418688, -0.081312]])
    inv = x.new_tensor([[1.0, 0.0, 1.402], [1.0, -0.344136, -0.714136], [1.0, 1.772, 0.0]])
    ycc = torch.einsum("oc,nchw->nohw", fwd, 255.0 * x.clamp(0, 1))

    def roundtrip(p, t):
        n, h, w = p.shape
        b = p.view(n, h // 8, 8, w // 8, 8).permute(0, 1, 3, 2, 4)
        c = torch.einsum("uy,nabyx,vx->nabuv", D, b, D)
        c = torch.round(c / (t * f)) * (t * f)
        return torch.einsum("uy,nabuv,vx->nabyx", D, c, D).permute(0, 1, 3, 2, 4).reshape(n, h, w)

    y = roundtrip(ycc[:, 0], T[0])
    cb, cr = (F.interpolate(roundtrip(F.avg_pool2d(ycc[:, i:i + 1], 2)[:, 0], T[1])[:, None], scale_factor=2, mode="nearest")[:, 0] for i in (1, 2))
    return (torch.einsum("oc,nchw->nohw", inv, torch.stack([y, cb, cr], 1)).clamp(0, 255) / 255.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--windows", type=int, default=5)
    args = ap.parse_args()
    import degrade_ref as R
    from instantir_amd import degrade as DG, lib, ops
    lib.load()
    if not torch.cuda.is_available():
        raise SystemExit("degrade_bench needs an MI355X")
    dev = torch.device("cuda:0")
    D = torch.from_numpy(R.DCT32).to(dev)
    T = torch.from_numpy(np.stack([R.T_LUMA, R.T_CHROMA]).astype(np.float32)).to(dev)
    taps21 = torch.from_numpy(DG.gaussian_kernel(21, 2.0, 1.0, 0.4).astype(np.float32))[None].to(dev)
    taps7 = torch.from_numpy(DG.gaussian_kernel(7, 1.0).astype(np.float32))[None].to(dev)
    tiny = torch.rand(1, 3, 16, 16, device=dev)
    tiny_out = torch.empty_like(tiny)
    sigma, quality = torch.tensor([10.0]), torch.tensor([75.0])
    for side in SIDES:
        x = torch.rand(1, 3, side, side, device=dev)
        out = torch.empty_like(x)
        legs = {
            "filter2d k21": lambda: ops.filter2d(x, taps21, out=out),
            "filter2d k21 empty": lambda: ops.filter2d(tiny, taps21, out=tiny_out),
            "filter2d k21 torch": lambda: torch_filter2d(x, taps21),
            "filter2d k7": lambda: ops.filter2d(x, taps7, out=out),
            "filter2d k7 empty": lambda: ops.filter2d(tiny, taps7, out=tiny_out),
            "filter2d k7 torch": lambda: torch_filter2d(x, taps7),
            "noise": lambda: ops.add_gaussian_noise(x, sigma, 1, out=out),
            "noise empty": lambda: ops.add_gaussian_noise(tiny, sigma, 1, out=tiny_out),
            "noise torch": lambda: (x + (10.0 / 255.0) * torch.randn_like(x)).clamp_(0, 1),
            "jpeg": lambda: ops.jpeg_roundtrip(x, quality, out=out),
            "jpeg empty": lambda: ops.jpeg_roundtrip(tiny, quality, out=tiny_out),
            "jpeg torch": lambda: torch_jpeg(x, 75.0, D, T),
        }
        us = {k: [] for k in legs}
        for _ in range(args.windows):
            for k, fn in legs.items():
                us[k].append(timed(fn, args.iters))
        med = {k: statistics.median(v) for k, v in us.items()}
        fb = 2 * 3 * side * side * 4
        fl = fb / (HBM_TBS * 1e12) * 1e6
        for k in ("filter2d k21", "filter2d k7", "noise", "jpeg"):
            print(f"{side}x{side} {k:12s}: {med[k]:8.1f} us (windows {min(us[k]):.1f} .. {max(us[k]):.1f}); empty call {med[k + ' empty']:.1f} us; "
                  f"byte floor {fb / 1e6:.1f} MB = {fl:.1f} us ({100 * fl / med[k]:.0f} % of it reached); torch composition "
                  f"{med[k + ' torch']:.1f} us ({med[k + ' torch'] / med[k]:.2f} x)", flush=True)
        # the compositions compute what the launches compute (the noise leg has another generator and is not compared)
        a, b = ops.filter2d(x, taps21), torch_filter2d(x, taps21)
        j, t = ops.jpeg_roundtrip(x, quality), torch_jpeg(x, 75.0, D, T)
        print(f"{side}x{side} agreement   : filter2d max |difference| {float((a - b).abs().max()):.2e}; jpeg {float(((j - t).abs() > 1e-4).float().mean()) * 100:.3f} % "
              f"of elements differ by more than 1e-4 (rounding flips)", flush=True)


if __name__ == "__main__":
    main()
