"""Device DISTS (instantir_amd.dists.DISTS, VGG-16 widths, synthetic weights, fp16) cost on one MI355X.

    python tools/dists_bench.py [--windows 5] [--iters 20]

Two parts, for one 3-channel uint8 pair at 1024^2 and one at 2048^2.
The three new launches on their own, at the stage shapes of the pair: `dists_stats` at the five stages, `dists_l2pool` at the four
pooled ones, `dists_image_stats` of the image; each beside an empty launch of the same entry (a 1 x 1 stage, a 16 x 16 image:
the same kernels, one workgroup) in alternating windows of `--iters` calls by device events, the median window of each, and
beside its byte floor over 6.29 TB/s (stats: the 2 H W C 16-bit values read once; l2pool: that and the quarter-size write;
image: the two sources read once).
Then the whole call `model(a, b)` (upload excluded, the read-back of the score included) beside `LPIPS` on the same pair in the
same process, alternating: both run the same thirteen convs, so the difference is the new kernels and the fp64 arithmetic on
their sums against the taps.  Nothing here is a pass bar."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_TBS = 6.29
SIDES = (1024, 2048)
WIDTHS = (64, 128, 256, 512, 512)


def window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def alternate(legs, windows, iters):
    """{name: fn} -> {name: (median, min, max) us per call} over `windows` alternating windows of `iters` calls, warm."""
    for fn in legs.values():
        fn()
    us = {k: [] for k in legs}
    for _ in range(windows):
        for k, fn in legs.items():
            us[k].append(window(fn, iters))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in us.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    from instantir_amd import dists as DS, lib, lpips as LP, ops
    lib.load()
    if not torch.cuda.is_available():
        raise SystemExit("dists_bench needs an MI355X: there is nothing to time on the host")
    dev = torch.device("cuda:0")
    model, lp = DS.DISTS.synthetic(0, device=dev), LP.LPIPS.synthetic(0, device=dev)
    rng = np.random.default_rng(0)
    tiny = torch.from_numpy(rng.integers(0, 255, (1, 16, 16, 3), dtype=np.uint8)).to(dev)
    for side in SIDES:
        a = torch.from_numpy(rng.integers(0, 255, (1, side, side, 3), dtype=np.uint8)).to(dev)
        b = (a.float() + 25 * torch.randn(a.shape, device=dev)).clamp(0, 255).to(torch.uint8)
        print(f"{side}x{side} pair, fp16", flush=True)
        sizes = model.stage_sizes(side, side)
        for k, C in enumerate(WIDTHS, 1):
            H, W = sizes[k]
            x = torch.randn(2 * H * W, C, device=dev, dtype=torch.float16)
            x1 = torch.randn(2, C, device=dev, dtype=torch.float16)
            ws = torch.empty(ops.dists_stats_workspace_bytes(1, H, W, C) // 8, dtype=torch.float64, device=dev)
            out = torch.empty(1, C, 5, dtype=torch.float64, device=dev)
            legs = {"stats": lambda: ops.dists_stats(x, 1, H, W, ws=ws, out=out), "stats_empty": lambda: ops.dists_stats(x1, 1, 1, 1, ws=ws, out=out)}
            nbytes = {"stats": x.numel() * 2}
            if k < 5:
                pooled = torch.empty(2 * ((H + 1) // 2) * ((W + 1) // 2), C, device=dev, dtype=torch.float16)
                legs["l2pool"] = lambda: ops.dists_l2pool(x, 2, H, W, out=pooled)
                legs["l2pool_empty"] = lambda: ops.dists_l2pool(x1, 2, 1, 1, out=pooled[:2])
                nbytes["l2pool"] = x.numel() * 2 + pooled.numel() * 2
            res = alternate(legs, args.windows, args.iters)
            for name, nb in nbytes.items():
                t, lo, hi = res[name]
                floor = nb / (HBM_TBS * 1e12) * 1e6
                print(f"  stage {k} {H}x{W}x{C} {name:6s}: {t:8.1f} us (windows {lo:.1f} .. {hi:.1f}); empty launch {res[name + '_empty'][0]:.1f} us; "
                      f"byte floor {nb / 1e6:.1f} MB = {floor:.1f} us, {t / floor:.2f} x the floor, {nb / t / 1e6:.2f} TB/s", flush=True)
            del x, ws, legs
        ws = torch.empty(ops.dists_image_stats_workspace_bytes(1, side, side) // 8, dtype=torch.float64, device=dev)
        out = torch.empty(1, 3, 5, dtype=torch.float64, device=dev)
        af = (a.float() / 255).permute(0, 3, 1, 2).contiguous()
        bf = (b.float() / 255).permute(0, 3, 1, 2).contiguous()
        res = alternate({"u8": lambda: ops.dists_image_stats(a, b, ws=ws, out=out), "fp32": lambda: ops.dists_image_stats(af, bf, ws=ws, out=out),
                         "empty": lambda: ops.dists_image_stats(tiny, tiny, ws=ws, out=out)}, args.windows, args.iters)
        for name, nb in (("u8", 2 * a.numel()), ("fp32", 2 * af.numel() * 4)):
            t, lo, hi = res[name]
            floor = nb / (HBM_TBS * 1e12) * 1e6
            print(f"  stage 0 {side}x{side}x3 image_stats {name}: {t:8.1f} us (windows {lo:.1f} .. {hi:.1f}); empty launch {res['empty'][0]:.1f} us; "
                  f"byte floor {nb / 1e6:.1f} MB = {floor:.1f} us, {t / floor:.2f} x the floor", flush=True)
        del af, bf
        res = alternate({"dists": lambda: model(a, b).cpu(), "lpips": lambda: lp(a, b).cpu(), "dists_empty": lambda: model(tiny, tiny).cpu(),
                         "lpips_empty": lambda: lp(tiny, tiny).cpu()}, args.windows, max(1, args.iters // 7))
        for name in ("dists", "lpips"):
            t, lo, hi = res[name]
            print(f"  {name} model(a, b): {t / 1e3:.2f} ms per call (windows {lo / 1e3:.2f} .. {hi / 1e3:.2f} ms); empty call {res[name + '_empty'][0]:.0f} us",
                  flush=True)
        print(f"  dists - lpips: {(res['dists'][0] - res['lpips'][0]) / 1e3:+.2f} ms; DISTS {float(model(a, b)[0]):.4f}, LPIPS {float(lp(a, b)[0]):.4f}", flush=True)


if __name__ == "__main__":
    main()
