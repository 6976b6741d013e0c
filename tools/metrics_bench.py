"""Device PSNR / SSIM (ops.image_metrics) cost on one MI355X, beside the host computation it replaces.

    python tools/metrics_bench.py [--iters 100]

One 3-channel image pair at 1024^2 and at 2048^2, sources uint8 / uint8 and fp32 / uint8 (a decoded tensor scored against an
uploaded ground truth, quantised): both figures, the MSE alone and the SSIM alone, by device events, warm, best of two
alternating windows of `--iters` calls; an empty call through the same wrapper (an 11 x 11 one-channel pair: the same two
launches, one workgroup each) the same way; the byte floor from the shapes (each source read once; the partial sums are a few
KiB) over 6.29 TB/s; and the wall time of the fp64 host restatement of tests/metrics_ref.py on the same pair, which is what a
user without this entry would run after downloading the image (`--host-iters` calls, the fastest)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--host-iters", type=int, default=1)
    args = ap.parse_args()
    import metrics_ref as R
    from instantir_amd import lib, ops
    lib.load()
    if not torch.cuda.is_available():
        raise SystemExit("metrics_bench needs an MI355X: there is nothing to time on the host but the restatement")
    dev = torch.device("cuda:0")
    tiny = torch.zeros(1, 11, 11, 1, dtype=torch.uint8, device=dev)
    for side in SIDES:
        a8, b8 = R.pair(side, (1, 3, side, side), True, True)
        a_u8, b_u8 = torch.from_numpy(a8).to(dev), torch.from_numpy(b8).to(dev)
        a_f32 = a_u8.permute(0, 3, 1, 2).float().div(255).contiguous()
        ws = torch.empty(1 << 20, dtype=torch.float64, device=dev)
        for form, a, q, a_bytes in (("uint8 / uint8", a_u8, (False, False), 1), ("fp32 / uint8", a_f32, (True, False), 4)):
            legs = {"both": lambda: ops.image_metrics(a, b_u8, quantize=q, ws=ws),
                    "psnr": lambda: ops.image_metrics(a, b_u8, quantize=q, what="psnr", ws=ws),
                    "ssim": lambda: ops.image_metrics(a, b_u8, quantize=q, what="ssim", ws=ws),
                    "empty": lambda: ops.image_metrics(tiny, tiny, ws=ws)}
            us = {k: 1e30 for k in legs}
            for _ in range(2):
                for k, fn in legs.items():
                    us[k] = min(us[k], timed(fn, args.iters))
            fb = 3 * side * side * (a_bytes + 1)
            fl = fb / (HBM_TBS * 1e12) * 1e6
            for k in ("both", "psnr", "ssim"):
                net = us[k] - us["empty"]
                net_txt = f"{100 * fl / net:.0f} % net of the empty call" if net > 1.0 else "no more than the empty call costs: issue-bound"
                print(f"{side}x{side} {form:13s} {k:4s}: {us[k]:7.1f} us for 2 launches (empty call {us['empty']:.1f} us), byte floor "
                      f"{fb / 1e6:.1f} MB = {fl:.1f} us ({100 * fl / us[k]:.0f} % of it reached; {net_txt})", flush=True)
        host = []
        for _ in range(args.host_iters):
            t0 = time.perf_counter()
            want = R.evaluate(a8, b8)
            host.append(time.perf_counter() - t0)
        got = ops.image_metrics(a_u8, b_u8).cpu().numpy()
        t0 = time.perf_counter()
        a_u8.cpu(), b_u8.cpu()
        down = time.perf_counter() - t0
        print(f"{side}x{side} host         : fp64 numpy restatement {min(host) * 1e3:.0f} ms (+ {down * 1e3:.2f} ms to download both images); "
              f"device against it: MSE {'equal' if got[0, 0] == want[0, 0] else 'DIFFERS'}, |SSIM difference| {abs(got[0, 1] - want[0, 1]):.2e}",
              flush=True)


if __name__ == "__main__":
    main()
