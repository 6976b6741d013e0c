"""FreeU cost per denoising step at BASELINE configs[1] geometry (1024x1024, batch 1, cfg 7 = 2 rows, previewer + Aggregator
step, hipGraph, two streams): alternating FreeU-off / FreeU-on legs on one pipeline, each warm, timed with device events.

    python tools/freeu_bench.py [--pairs 3] [--steps 20] [--warmup 5] [--size 1024]

Prints one line per leg and the medians; the FreeU factors are diffusers' SDXL values (0.9, 0.2, 1.3, 1.4).

    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/freeu_bench.py --kernels 50

launches, at each concat shape of the 1024^2 step (R = 2), the two copy_add launches of the FreeU-off concat and the
freeu_stats + freeu_concat pair of the FreeU-on concat, `--kernels` times each, for a per-kernel time table."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--kernels", type=int, default=0, help="only launch the per-shape kernels this many times (for rocprofv3)")
    args = ap.parse_args()
    if args.kernels:
        return kernels(args.kernels)
    from instantir_amd import lib, weights as W
    from instantir_amd.config import UNetConfig
    from instantir_amd.pipeline import InstantIRPipeline, _DenoiseLoop
    from instantir_amd.schedulers import DDIMScheduler, LCMSingleStepScheduler
    lib.load()
    dev = torch.device("cuda:0")
    cfg = UNetConfig.sdxl()
    Hl, B, rep = args.size // 8, 1, 2
    sd = W.synth_state_dict(W.unet_specs(cfg), 1234, device=dev)
    pipe = InstantIRPipeline(cfg, sd, scheduler=DDIMScheduler(), device=dev)
    pipe.aggregator.load_state_dict(W.synth_state_dict(W.aggregator_specs(cfg), 1235, device=dev))
    pipe.prepare_previewers(W.synth_state_dict(W.lora_specs(cfg), 1236, device=dev), lora_alpha=cfg.lora_rank // 8)
    pipe._build()
    g = torch.Generator().manual_seed(42)
    lq = (torch.randn(B, 4, Hl, Hl, generator=g) * 0.8).to(dev)
    ctx = torch.randn(rep * B, cfg.text_len, cfg.cross_attention_dim, generator=g)
    pl = torch.randn(rep * B, cfg.pooled_dim, generator=g)
    img = torch.randn(2, B, cfg.resampler.seq_len, cfg.resampler.embedding_dim, generator=g)
    px = Hl * 8
    time_ids = torch.tensor([[px, px, 0, 0, px, px]], dtype=torch.float32).repeat(rep * B, 1)
    lcm = LCMSingleStepScheduler.from_config(pipe.scheduler.config)
    pipe.scheduler.set_timesteps(30)
    ts = [int(t) for t in pipe.scheduler.timesteps]
    x0 = pipe.scheduler.add_noise(lq, torch.randn(lq.shape, generator=g).to(dev), torch.tensor([ts[0]] * B)).contiguous()
    scale_rows = torch.ones(rep * B)

    def leg(freeu):
        if freeu is None:
            pipe.disable_freeu()
        else:
            pipe.enable_freeu(*freeu)
        pipe._build()
        st = pipe._unet.prepare(ctx, pl, time_ids, pipe._unet.resampler(img), Hl, Hl)
        st_prev = pipe._unet_prev.prepare(ctx, pl, time_ids, pipe._unet_prev.resampler(img), Hl, Hl)
        st_agg = pipe._agg.prepare(pl, time_ids, Hl, Hl)
        loop = _DenoiseLoop(pipe, B, rep, Hl, Hl, st, st_prev, st_agg, lq, None, lcm)
        x = x0.clone()
        for i in range(args.warmup):
            loop.step("preview", ts[i % len(ts)], x, scale_rows, 7.0, 0.0, None, None)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(args.steps):
            loop.step("preview", ts[(args.warmup + i) % len(ts)], x, scale_rows, 7.0, 0.0, None, None)
        e1.record()
        torch.cuda.synchronize()
        finite = bool(torch.isfinite(x).all().item())
        del loop
        return e0.elapsed_time(e1) / args.steps, finite

    res = {"off": [], "on": []}
    for p in range(args.pairs):
        for name, f in (("off", None), ("on", (0.9, 0.2, 1.3, 1.4))):
            ms, finite = leg(f)
            res[name].append(ms)
            print(f"pair {p + 1} {name:3s} ms_per_step {ms:.3f} finite {finite}", flush=True)
    mo, mn = statistics.median(res["off"]), statistics.median(res["on"])
    print(f"median off {mo:.3f} on {mn:.3f} ms/step: FreeU costs {mn - mo:+.3f} ms/step ({args.size}^2, cfg 7, preview step)")


def kernels(n):
    from instantir_amd import lib, ops
    lib.load()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(3)
    rnd = lambda *s: torch.randn(*s, generator=g).half().to(dev)
    sc = torch.tensor([0.8, 1.1], device=dev)
    # (H, W, hidden cx, skip cs): up_blocks.0 and up_blocks.1 of the 1024^2 step
    for H, W, cx, cs in [(32, 32, 1280, 1280), (32, 32, 1280, 640), (64, 64, 1280, 640), (64, 64, 640, 640), (64, 64, 640, 320)]:
        rows = 2 * H * W
        x, sk, add = rnd(rows, cx), rnd(rows, cs), rnd(rows, cs)
        cat = torch.empty(rows, cx + cs, dtype=torch.half, device=dev)
        parts = torch.empty(ops.freeu_partials_floats(rows, H, W, cs), dtype=torch.float32, device=dev)
        def off():
            ops.copy_add(x, cat, 0, rows_per_scale=H * W)
            ops.copy_add(sk, cat, cx, add=add, add_scale=sc, rows_per_scale=H * W)

        def on():
            ops.freeu_stats(sk, parts, H, W, add=add, add_scale=sc)
            ops.freeu_concat(x, sk, cat, parts, H, W, 1.3, 0.9, add=add, add_scale=sc)
        us = {}
        for name, fn in (("copy_add pair", off), ("freeu pair", on), ("copy_add pair ", off), ("freeu pair ", on)):
            fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            torch.cuda.synchronize()
            us[name.strip()] = min(us.get(name.strip(), 1e30), e0.elapsed_time(e1) * 1e3 / n)
        print(f"{H}x{W} cx={cx} cs={cs}: copy_add pair {us['copy_add pair']:.2f} us, freeu stats+concat {us['freeu pair']:.2f} us "
              f"({us['freeu pair'] / us['copy_add pair']:.2f}x)", flush=True)


if __name__ == "__main__":
    main()
