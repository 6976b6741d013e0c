"""Device LPIPS (instantir_amd.lpips.LPIPS, VGG-16 widths, synthetic weights, fp16) cost on one MI355X.

    python tools/lpips_bench.py [--windows 5] [--iters 3]

One 3-channel uint8 pair at 1024^2 and one at 2048^2.  The whole call `model(a, b)` (upload excluded, the read-back of five
numbers included) and an empty call (a 16 x 16 pair: the same 28 launches, a workgroup or a few each) by device events, warm, in
alternating windows of `--iters` calls, the median window of each.  Then every launch of one call between its own pair of
events (median over `--windows` calls; events between launches add issue gaps, so these are upper ends), summed by kind beside
what the shapes say: the convs' FLOP count (2 x rows x Cout x 9 x Cin, the first conv at its 3 real input channels) and the
byte floor of the new kernels (prep: the source read and the 64-channel rows written; relu: the matrix read and written; tap:
the pre-activations read and the pooled quarter written) over 6.29 TB/s.  Nothing here is a pass bar."""
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


def window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


class TimedOps:
    """`ops` with a pair of events around every launch the LPIPS module makes; `take()` -> [(entry, us, flop, bytes)]."""

    def __init__(self, ops):
        self._ops, self.log = ops, []

    def __getattr__(self, name):
        fn = getattr(self._ops, name)
        if name not in ("lpips_prep", "relu_", "conv2d", "lpips_tap"):
            return fn

        def timed(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*a, **k)
            e1.record()
            flop = nbytes = 0
            if name == "conv2d":
                x, w = a[0], a[1]
                cin = w.shape[3] if self.log_has_conv() else 3          # a call's first conv reads the 3-channel image, zero padded
                flop = 2 * x.shape[0] * x.shape[1] * x.shape[2] * w.shape[0] * 9 * cin
            elif name == "lpips_prep":
                src, o = a[0], a[1]
                nbytes = src.numel() * src.element_size() + o.shape[0] * self._ops.LPIPS_CPAD * 2
            elif name == "relu_":
                nbytes = 2 * a[0].numel() * 2
            else:
                x, pooled = a[0], k.get("pooled")
                nbytes = x.numel() * 2 + (0 if pooled is None else pooled.numel() * 2)
            self.log.append((name, e0, e1, flop, nbytes))
            return out
        return timed

    def log_has_conv(self):
        return any(n == "conv2d" for n, *_ in self.log)

    def take(self):
        torch.cuda.synchronize()
        out = [(n, e0.elapsed_time(e1) * 1e3, fl, nb) for n, e0, e1, fl, nb in self.log]
        self.log = []
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    args = ap.parse_args()
    from instantir_amd import lib, lpips as LP, ops, vgg as VG
    lib.load()
    if not torch.cuda.is_available():
        raise SystemExit("lpips_bench needs an MI355X: there is nothing to time on the host")
    dev = torch.device("cuda:0")
    model = LP.LPIPS.synthetic(0, device=dev)
    rng = np.random.default_rng(0)
    tiny = torch.from_numpy(rng.integers(0, 255, (1, 16, 16, 3), dtype=np.uint8)).to(dev)
    for side in SIDES:
        a = torch.from_numpy(rng.integers(0, 255, (1, side, side, 3), dtype=np.uint8)).to(dev)
        b = (a.float() + 25 * torch.randn(a.shape, device=dev)).clamp(0, 255).to(torch.uint8)
        legs = {"pair": lambda: model(a, b).cpu(), "empty": lambda: model(tiny, tiny).cpu()}
        for fn in legs.values():
            fn()
        us = {k: [] for k in legs}
        for _ in range(args.windows):
            for k, fn in legs.items():
                us[k].append(window(fn, args.iters))
        total, empty = statistics.median(us["pair"]), statistics.median(us["empty"])
        print(f"{side}x{side} pair, fp16: {total / 1e3:.2f} ms per call (windows {min(us['pair']) / 1e3:.2f} .. {max(us['pair']) / 1e3:.2f} ms); "
              f"empty call {empty:.0f} us; score {float(model(a, b)[0]):.4f}", flush=True)
        timed = TimedOps(ops)
        LP.ops = VG.ops = timed              # (the tap is launched from lpips.py, the trunk from vgg.py)
        try:
            runs = []
            for _ in range(args.windows):
                model(a, b)
                runs.append(timed.take())
        finally:
            LP.ops = VG.ops = ops
        launches = [(runs[0][i][0], statistics.median(r[i][1] for r in runs), runs[0][i][2], runs[0][i][3]) for i in range(len(runs[0]))]
        summed = sum(t for _, t, _, _ in launches)
        for kind in ("conv2d", "lpips_prep", "relu_", "lpips_tap"):
            sel = [x for x in launches if x[0] == kind]
            t, fl, nb = sum(x[1] for x in sel), sum(x[2] for x in sel), sum(x[3] for x in sel)
            if kind == "conv2d":
                print(f"  {kind:10s} x{len(sel):2d}: {t / 1e3:8.3f} ms, {fl / 1e12:.3f} TFLOP -> {fl / t / 1e6:.0f} TFLOP/s; "
                      f"{100 * t / summed:.1f} % of the summed launches", flush=True)
            else:
                floor = nb / (HBM_TBS * 1e12) * 1e6
                print(f"  {kind:10s} x{len(sel):2d}: {t / 1e3:8.3f} ms, byte floor {nb / 1e6:.1f} MB = {floor / 1e3:.3f} ms "
                      f"({100 * floor / t:.0f} % of it reached); {100 * t / summed:.1f} % of the summed launches", flush=True)
        print(f"  summed launches {summed / 1e3:.2f} ms of the {total / 1e3:.2f} ms call", flush=True)
        for name, t, fl, nb in launches:
            what = f"{fl / 1e9:9.1f} GFLOP {fl / t / 1e6:6.0f} TFLOP/s" if fl else f"{nb / 1e6:9.1f} MB    {nb / t / 1e6:6.2f} TB/s"
            print(f"    {name:10s} {t:9.1f} us  {what}", flush=True)


if __name__ == "__main__":
    main()
