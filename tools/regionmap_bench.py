"""Restore-map launches (restore_map: block-maximum pool, pixel composite) on one MI355X.

    python tools/regionmap_bench.py [--sizes 1024 2048] [--iters 200] [--feather 4]

per size (B = 1, 3 channels), device events, best of two windows of `--iters` calls: iir_map_pool_max_f32 (factor 8) and
iir_region_composite_f32 (out of place and in place), each against its byte floor from the shapes over 6.29 TB/s (the
float4-copy bandwidth measured on this chip):
  pool:      the pixel map in, the latent map out;
  composite: the map in and the uint16 row counts out, then the counts, decoded and original in and the result out.
The step with a map is timed by tools/sched_bench.py --map."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

HBM_TBS = 6.29


def timed(fn, n):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def best(fns, n, windows=2):
    us = {k: 1e30 for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():                                    # alternating
            us[k] = min(us[k], timed(fn, n))
    return us


def kernels(sizes, n, r):
    from instantir_amd import lib, ops
    h = lib.load()
    dev = torch.device("cuda:0")
    for size in sizes:
        g = torch.Generator().manual_seed(size)
        dec, orig = torch.rand(1, 3, size, size, generator=g).to(dev), torch.rand(1, 3, size, size, generator=g).to(dev)
        m = torch.zeros(1, size, size)
        m[:, :, size // 2:] = 1.0
        m[:, size // 4:size // 2, :size // 4] = 0.5
        m = m.to(dev)
        out, inplace = torch.empty_like(dec), dec.clone()
        pooled = torch.empty(1, size // 8, size // 8, device=dev)
        ws = torch.empty(h.iir_region_composite_workspace_bytes(1, size, size), dtype=torch.uint8, device=dev)
        px = size * size
        floor = {"pool": 4 * px + 4 * px // 64, "composite": (4 * px + 2 * px) + (2 * px + 3 * 3 * 4 * px)}
        us = best({"pool": lambda: ops.map_pool_max(m, 8, out=pooled),
                   "composite": lambda: ops.region_composite(dec, orig, m, r, out=out, ws=ws),
                   "composite in place": lambda: ops.region_composite(inplace, orig, m, r, out=inplace, ws=ws)}, n)
        for name, t in us.items():
            fb = floor[name.split()[0]]
            fl = fb / (HBM_TBS * 1e12) * 1e6
            print(f"{name:18s} {size}x{size} B=1 r={r}: {t:.1f} us, byte floor {fb / 1e6:.1f} MB = {fl:.1f} us "
                  f"({100 * fl / t:.0f} % of it reached)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 2048])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--feather", type=int, default=4)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("regionmap_bench needs an MI355X")
    kernels(args.sizes, args.iters, args.feather)


if __name__ == "__main__":
    main()
