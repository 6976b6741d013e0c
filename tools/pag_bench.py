"""Perturbed-attention guidance (PAG) cost per denoising step at BASELINE configs[1] geometry (1024x1024, batch 1, cfg 7, DDPM,
previewer + Aggregator step, hipGraph, two streams): alternating legs PAG off / `mid` / `mid` + `up_blocks.0` on one pipeline,
each warm, timed with device events.  PAG on runs the main UNet on 3 rows instead of 2, and does not defer the shallow SFT
heads to the side stream; the leg `off-nodefer` is PAG off without that deferral, the share of the PAG cost it explains.

    python tools/pag_bench.py [--rounds 3] [--steps 20] [--warmup 5] [--size 1024]

Prints one line per leg and the medians.

    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/pag_bench.py --kernels 50

launches, at the step's two self-attention shapes (T = 4096 x 10 heads, T = 1024 x 20 heads), the plain 2-row launch and the
3-row launch with the third row the identity (iir_attention_d64_ident_f16), `--kernels` times each; prints event timings too."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

LEGS = (("off", None), ("off-nodefer", None), ("mid", "mid"), ("mid+up0", ["mid", "up_blocks.0"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--kernels", type=int, default=0, help="only launch the attention shapes this many times (for rocprofv3)")
    args = ap.parse_args()
    if args.kernels:
        return kernels(args.kernels)
    from instantir_amd import lib, weights as W
    from instantir_amd.config import UNetConfig
    from instantir_amd.pipeline import InstantIRPipeline, _DenoiseLoop
    from instantir_amd.schedulers import DDPMScheduler, LCMSingleStepScheduler
    lib.load()
    dev = torch.device("cuda:0")
    cfg = UNetConfig.sdxl()
    Hl, B, rep = args.size // 8, 1, 2
    sd = W.synth_state_dict(W.unet_specs(cfg), 1234, device=dev)
    pipe = InstantIRPipeline(cfg, sd, scheduler=DDPMScheduler(), device=dev)
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

    def leg(name, layers):
        on = layers is not None
        pipe.overlap_sft = name != "off-nodefer"
        if on:
            pipe.enable_pag(layers)
            pipe._unet.set_pag(pipe._pag_paths, rep * B)
        else:
            pipe.disable_pag()
            pipe._unet.set_pag(None, 0)
        groups = rep + int(on)
        st = pipe._main_state(ctx, pl, time_ids, img, Hl, Hl, B, rep, on)
        st_prev = pipe._unet_prev.prepare(ctx, pl, time_ids, pipe._unet_prev.resampler(img), Hl, Hl)
        st_agg = pipe._agg.prepare(pl, time_ids, Hl, Hl, out_rows=groups * B if on else None)
        loop = _DenoiseLoop(pipe, B, rep, Hl, Hl, st, st_prev, st_agg, lq, None, lcm, pag_on=on)
        scale_rows = torch.ones(groups * B)
        x = x0.clone()
        for i in range(args.warmup):
            loop.step("preview", ts[i % len(ts)], x, scale_rows, 7.0, 0.0, None, None, pag_s=3.0)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(args.steps):
            loop.step("preview", ts[(args.warmup + i) % len(ts)], x, scale_rows, 7.0, 0.0, None, None, pag_s=3.0)
        e1.record()
        torch.cuda.synchronize()
        finite = bool(torch.isfinite(x).all().item())
        del loop
        return e0.elapsed_time(e1) / args.steps, finite

    res = {name: [] for name, _ in LEGS}
    for r in range(args.rounds):
        for name, layers in LEGS:
            ms, finite = leg(name, layers)
            res[name].append(ms)
            print(f"round {r + 1} {name:11s} ms_per_step {ms:.3f} finite {finite}", flush=True)
    med = {k: statistics.median(v) for k, v in res.items()}
    print("median " + " ".join(f"{k} {v:.3f}" for k, v in med.items()) + f" ms/step ({args.size}^2, cfg 7, DDPM, preview step)")
    for k in ("off-nodefer", "mid", "mid+up0"):
        print(f"{k}: {med[k] - med['off']:+.3f} ms/step, {med[k] / med['off']:.3f}x PAG off")


def kernels(n):
    from instantir_amd import lib, ops
    lib.load()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(3)
    for T, heads in [(4096, 10), (1024, 20)]:
        C = heads * 64
        qk3 = (torch.randn(3 * T, 2 * C, generator=g) * 0.5).half().to(dev)
        vt3 = torch.randn(C, 3 * T, generator=g).half().to(dev)
        o3 = torch.empty(3 * T, C, dtype=torch.half, device=dev)
        # 2-row plain launch on the first two rows (same buffers, batch strides of the 3-row layout)
        plain = lambda: ops.attention(qk3[:, :C], o3, [(qk3[:, C:], T, vt3, T, T)], 2, heads, T, q_prescaled=True)
        ident = lambda: ops.attention(qk3[:, :C], o3, [(qk3[:, C:], T, vt3, T, T)], 3, heads, T, q_prescaled=True, ident_from=2)
        us = {}
        for name, fn in (("plain2", plain), ("ident3", ident), ("plain2 ", plain), ("ident3 ", ident)):
            fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            torch.cuda.synchronize()
            us[name.strip()] = min(us.get(name.strip(), 1e30), e0.elapsed_time(e1) * 1e3 / n)
        print(f"T={T} heads={heads}: plain 2-row {us['plain2']:.2f} us, 3-row with identity row {us['ident3']:.2f} us "
              f"({us['ident3'] / us['plain2']:.3f}x)", flush=True)


if __name__ == "__main__":
    main()
