"""Device NIQE statistics (ops.niqe_stats) cost on one MI355X, beside the host computation they replace.

    python tools/niqe_bench.py [--iters 100]
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/niqe_bench.py --kernels 50

One 3-channel image at 1024^2 and at 2048^2, as uint8 and as fp32: the call (four launches: grey, half-size, one per scale) by
device events, warm, best of two alternating windows of `--iters` calls; an empty call through the same wrapper (a 96 x 192
one-channel image: the same four launches, two workgroups each in the block launches) the same way; the host's share of a
score (`niqe.features` and the distance on the downloaded sums); the byte floor from the shapes (the source read once, the two
fp32 grey planes written once and read once; the sums are a few KiB) over 6.29 TB/s; and the wall time of the fp64 host
restatement of tests/niqe_ref.py on the same image.  `--kernels N` only launches the 1024^2 and 2048^2 uint8 calls N times each,
for a kernel trace that gives every launch's own duration."""
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
    ap.add_argument("--kernels", type=int, default=0, help="only launch the HIP kernels this many times (for rocprofv3)")
    args = ap.parse_args()
    import niqe_ref as R
    from instantir_amd import lib, niqe as NQ, ops
    lib.load()
    if not torch.cuda.is_available():
        raise SystemExit("niqe_bench needs an MI355X: there is nothing to time on the host but the restatement")
    dev = torch.device("cuda:0")
    tiny = torch.zeros(1, 96, 192, 1, dtype=torch.uint8, device=dev)
    model = NQ.NIQE(np.zeros(36), np.eye(36))
    for side in SIDES:
        u8 = R.picture(side, 1, 3, side, side)
        t_u8 = torch.from_numpy(u8).to(dev)
        t_f32 = torch.from_numpy(R.as_f32(u8)).to(dev)
        ws = torch.empty(side * side, dtype=torch.float64, device=dev)
        if args.kernels:
            for _ in range(args.kernels):
                ops.niqe_stats(t_u8, ws=ws)
            torch.cuda.synchronize()
            continue
        grid = (side // 96) * 96
        blocks = (side // 96) ** 2
        for form, t, src_bytes in (("uint8", t_u8, 1), ("fp32", t_f32, 4)):
            legs = {"call": lambda: ops.niqe_stats(t, ws=ws), "empty": lambda: ops.niqe_stats(tiny, ws=ws)}
            us = {k: 1e30 for k in legs}
            for _ in range(2):
                for k, fn in legs.items():
                    us[k] = min(us[k], timed(fn, args.iters))
            fb = 3 * grid * grid * src_bytes + 2 * (grid * grid + grid * grid // 4) * 4
            fl = fb / (HBM_TBS * 1e12) * 1e6
            net = us["call"] - us["empty"]
            print(f"{side}x{side} {form:5s}: {us['call']:7.1f} us for 4 launches over {blocks} blocks (empty call {us['empty']:.1f} us), byte "
                  f"floor {fb / 1e6:.1f} MB = {fl:.1f} us ({100 * fl / us['call']:.0f} % of it reached; {100 * fl / max(net, 1e-3):.0f} % net of "
                  "the empty call)", flush=True)
        stats = ops.niqe_stats(t_u8, ws=ws)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = stats.cpu().numpy()
        model.score_features(NQ.features(got))
        host_share = time.perf_counter() - t0
        host = []
        for _ in range(args.host_iters):
            t0 = time.perf_counter()
            want = R.stats(u8)
            host.append(time.perf_counter() - t0)
        sums = [c for c in range(26) if c % 5 > 1 or c == 25]
        rel = np.abs(got[..., sums] - want[..., sums]) / np.abs(want[..., sums])
        print(f"{side}x{side} host : the fit, the features and the distance from the downloaded sums {host_share * 1e3:.1f} ms; fp64 numpy "
              f"restatement of the sums {min(host) * 1e3:.0f} ms; device against it: largest relative difference of a sum {rel.max():.2e}, "
              f"of a count {np.abs(got[..., [0, 1]] - want[..., [0, 1]]).max():.0f}", flush=True)


if __name__ == "__main__":
    main()
