"""LQ fidelity guidance: what the launch (`ops.lq_fidelity`) costs.

    python tools/lq_fidelity_bench.py [--launches 400] [--windows 5]

    iir_lq_fidelity_f32 alone at 128^2 and 256^2 latents (B = 1, with the history plane) for sigma 0, 1.5 and 8: microseconds per
    launch (device events around n back-to-back launches, median of alternating windows), against the launch's byte floor --
    reads of x0 and the LQ latent, read-modify-write of prev, writes of x0' and the history plane, 6 fp32 planes, at the
    chip's 8 TB/s -- and against an empty launch (one workgroup of iir_lq_fidelity_f32's own radius-0 kernel on 1 element).

Prints one line per figure and a JSON summary."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_US = 8.0e6          # 8 TB/s


def timed_us(fn, n):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def kernel_leg(n=400, windows=5):
    from instantir_amd import lq_fidelity as lqf
    from instantir_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    legs, floors = {}, {}
    one = [torch.zeros(1, 1, 1, 1, device=dev) for _ in range(5)]
    wc = torch.tensor([0.75, 0.625], device=dev)
    legs["empty launch"] = lambda: ops.lq_fidelity(one[0], one[1], wc, one[2], one[3], hist=one[4])
    for Hl in (128, 256):
        x0, z, prev, hist = (torch.randn(1, 4, Hl, Hl, generator=g).to(dev) for _ in range(4))
        out = torch.empty_like(x0)
        for sigma in (0.0, 1.5, 8.0):
            t = lqf.taps(sigma)
            taps = torch.tensor(t, dtype=torch.float64).float().to(dev) if t else None
            name = f"{Hl}^2 sigma {sigma:g}"
            legs[name] = (lambda x0=x0, z=z, prev=prev, out=out, taps=taps, hist=hist:
                          ops.lq_fidelity(x0, z, wc, prev, out, taps=taps, hist=hist))
            floors[name] = 6 * x0.numel() * 4 / HBM_BYTES_PER_US
    samples = {k: [] for k in legs}
    for _ in range(windows):
        for k, fn in legs.items():
            samples[k].append(timed_us(fn, n))
    out = {}
    for k, v in samples.items():
        med = statistics.median(v)
        out[k] = {"us": round(med, 3), "min": round(min(v), 3), "max": round(max(v), 3)}
        if k in floors:
            out[k]["byte_floor_us"] = round(floors[k], 3)
        print(f"iir_lq_fidelity_f32 {k:18s} {med:8.2f} us (windows {min(v):.2f} .. {max(v):.2f})"
              + (f", byte floor {floors[k]:.2f} us" if k in floors else ""), flush=True)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=400, help="back-to-back launches per window")
    ap.add_argument("--windows", type=int, default=5)
    a = ap.parse_args()
    print(json.dumps({"kernel": kernel_leg(a.launches, a.windows)}))
