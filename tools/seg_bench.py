"""Smoothed-energy guidance (SEG) cost per denoising step at BASELINE configs[1] geometry (1024x1024, batch 1, cfg 7, DDPM,
previewer + Aggregator step, hipGraph, two streams): alternating legs off / PAG `mid` / SEG `mid` / SEG `mid` + `up_blocks.0` on
one pipeline, each warm, timed with device events (the legs and the timing of tools/pag_bench.py).

    python tools/seg_bench.py [--rounds 3] [--steps 20] [--warmup 5] [--size 1024] [--sigma 100]

Prints one line per leg and the medians.

    python tools/seg_bench.py --kernels 200

times iir_seg_blur_q_f16 alone at the two SDXL shapes of a 1024^2 step (one perturbed row: 32 x 32 tokens x 1280 channels and
64 x 64 x 640, sigma 100 and the mean mode) with device events over back-to-back launches, best of three windows, against its
byte floor: the perturbed Q read once and written once."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

LEGS = (("off", None, None), ("pag-mid", "pag", "mid"), ("seg-mid", "seg", "mid"), ("seg-mid+up0", "seg", ["mid", "up_blocks.0"]))
HBM_GBS = 8000.0            # MI355X peak HBM3E bandwidth, for the floor


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--sigma", type=float, default=100.0)
    ap.add_argument("--kernels", type=int, default=0, help="only launch the blur at the step's shapes this many times per window")
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

    def leg(kind, layers):
        on = kind is not None
        pipe.disable_pag()
        pipe.disable_seg()
        pipe._unet.set_pag(None, 0)
        pipe._unet.set_seg(None, 0)
        if kind == "pag":
            pipe.enable_pag(layers)
            pipe._unet.set_pag(pipe._pag_paths, rep * B)
        elif kind == "seg":
            pipe.enable_seg(layers, seg_blur_sigma=args.sigma)
            pipe._unet.set_seg(pipe._seg_paths, rep * B, args.sigma, Hl, Hl)
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

    res = {name: [] for name, _, _ in LEGS}
    for r in range(args.rounds):
        for name, kind, layers in LEGS:
            ms, finite = leg(kind, layers)
            res[name].append(ms)
            print(f"round {r + 1} {name:12s} ms_per_step {ms:.3f} finite {finite}", flush=True)
    med = {k: statistics.median(v) for k, v in res.items()}
    print("median " + " ".join(f"{k} {v:.3f}" for k, v in med.items()) + f" ms/step ({args.size}^2, cfg 7, DDPM, preview step, sigma {args.sigma:g})")
    for k in ("pag-mid", "seg-mid", "seg-mid+up0"):
        print(f"{k}: {med[k] - med['off']:+.3f} ms/step, {med[k] / med['off']:.3f}x off")


def kernels(n):
    from instantir_amd import lib, ops, seg
    lib.load()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(3)
    for H, C in [(32, 1280), (64, 640)]:
        T = H * H
        qk = (torch.randn(3 * T, 2 * C, generator=g) * 0.5).half().to(dev)          # the step's 3-row q | k buffer; row 2 is perturbed
        q = qk[2 * T:, :C]
        w = torch.tensor(seg.weights(100.0, H), dtype=torch.float64).float().to(dev)
        floor_us = 2 * T * C * 2 / (HBM_GBS * 1e3)
        for name, fn in (("sigma 100", lambda: ops.seg_blur_q(q, 1, H, H, w, w)), ("mean", lambda: ops.seg_blur_q(q, 1, H, H, mean=True))):
            best = 1e30
            for _ in range(3):
                fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(n):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                best = min(best, e0.elapsed_time(e1) * 1e3 / n)
            what = f"{name} ({len(w)} taps per axis)" if name != "mean" else "mean mode"
            print(f"{H}x{H} tokens x {C} channels, {what}: {best:.2f} us per launch; byte floor "
                  f"{2 * T * C * 2 / 1e6:.2f} MB = {floor_us:.2f} us at {HBM_GBS / 1e3:.0f} TB/s", flush=True)


if __name__ == "__main__":
    main()
