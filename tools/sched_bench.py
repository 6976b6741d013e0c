"""Per-scheduler denoising cost through InstantIRPipeline.__call__ (synthetic weights, latent in / latent out, CFG,
previewer + Aggregator every step, hipGraph replay).

    python tools/sched_bench.py [--size 1024] [--pairs 3] [--tiny]

Prints one line per timed call and a JSON summary:
  * ms/step of ddpm, euler and dpmpp_2m at `--steps` steps each, interleaved over `--pairs` rounds (the first call of each
    scheduler builds and captures its loop and is not timed);
  * wall time of a 20-step DPM++ 2M Karras call against a 30-step DDPM call.

    python tools/sched_bench.py --map [--size 1024] [--pairs 3] [--steps 20]

The restore map (restore_map=): the step launch alone, iir_sched_step without and with the IIR_STEP_KEEP group (the leg labelled
iir_sched_step_keep) at the step's shapes (B = 1, cfg, DDPM noise; device events, alternating windows), and DDPM calls through the pipeline without and with a map,
alternating pairs, ms/step medians.

    python tools/sched_bench.py --apg [--size 1024] [--pairs 3] [--steps 20]

Adaptive projected guidance (enable_apg): iir_sched_step against iir_apg_project + iir_sched_step with the IIR_STEP_APG group (the
leg labelled iir_sched_step_apg) at B = 1 and B = 8 (cfg, DDPM noise; device events, alternating windows), and DDPM calls through the pipeline with APG off and on, alternating pairs,
ms/step medians.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed_us(fn, n):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def map_launch_leg(size, n=500, windows=3):
    """iir_sched_step without and with the keep group on one stream, back to back: each figure includes the launch boundary.  The map
    adds three fp32 reads per latent element (map, LQ latent, seed noise) to x, eps and noise in, prev out."""
    from instantir_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    Hl = size // 8
    x = (torch.randn(1, 4, Hl, Hl, generator=g) * 0.8).to(dev)
    eps = torch.randn(2 * Hl * Hl, 64, generator=g).half().to(dev)
    lq, n0, nz = (torch.randn(1, 4, Hl, Hl, generator=g).to(dev) for _ in range(3))
    m = torch.rand(1, Hl * Hl, generator=g).to(dev)
    prev = torch.empty_like(x)
    coef = torch.tensor([7.0, 0.9, 0.3, 0.8, 0.5, 0.0, 0.1, 0.0], device=dev)
    kcoef = torch.tensor([0.5, 0.8, 0.6, 0.0], device=dev)
    legs = {"iir_sched_step": lambda: ops.sched_step(eps, 1, coef, x, prev, noise=nz),
            "iir_sched_step_keep": lambda: ops.sched_step(eps, 1, coef, x, prev, noise=nz, keep=(m, lq, n0, kcoef))}
    us = {k: [] for k in legs}
    for _ in range(windows):
        for k, fn in legs.items():
            us[k].append(timed_us(fn, n))
    for k, v in us.items():
        print(f"step launch {size}^2 (B=1, cfg, DDPM noise) {k}: windows {[round(t, 2) for t in v]} us, best {min(v):.2f} us", flush=True)
    return {k: round(min(v), 2) for k, v in us.items()}


def apg_launch_leg(size, B, n=500, windows=3):
    """iir_sched_step against iir_apg_project + iir_sched_step with the APG group on one stream, back to back: each figure includes
    the launch boundaries (two for APG).  APG adds one reduction pass (both eps row groups and x in, the average plane in and out) and one
    fp32 read per latent element in the step (the average; the uncond rows are no longer read there)."""
    from instantir_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    Hl = size // 8
    x = (torch.randn(B, 4, Hl, Hl, generator=g) * 0.8).to(dev)
    eps = torch.randn(2 * B * Hl * Hl, 64, generator=g).half().to(dev)
    nz = torch.randn(B, 4, Hl, Hl, generator=g).to(dev)
    avg, sa, ws = torch.zeros_like(x), torch.zeros(2 * B, device=dev), ops.apg_workspace(B, dev)
    prev = torch.empty_like(x)
    coef = torch.tensor([7.0, 0.9, 0.3, 0.8, 0.5, 0.0, 0.1, 0.0], device=dev)
    par = torch.tensor([0.0, 15.0, -0.5, 0.0], device=dev)

    def apg():
        ops.apg_project(eps, B, coef, x, (avg, sa, par), ws)
        ops.sched_step(eps, B, coef, x, prev, noise=nz, apg=(avg, sa, par))
    legs = {"iir_sched_step": lambda: ops.sched_step(eps, B, coef, x, prev, noise=nz),
            "iir_apg_project": lambda: ops.apg_project(eps, B, coef, x, (avg, sa, par), ws),
            "iir_apg_project + iir_sched_step_apg": apg}
    us = {k: [] for k in legs}
    for _ in range(windows):
        for k, fn in legs.items():
            avg.zero_()                      # the average is a geometric series under momentum -0.5: bounded, but start each window alike
            us[k].append(timed_us(fn, n))
    for k, v in us.items():
        print(f"step launch {size}^2 (B={B}, cfg, DDPM noise) {k}: windows {[round(t, 2) for t in v]} us, best {min(v):.2f} us", flush=True)
    return {k: round(min(v), 2) for k, v in us.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--tiny", action="store_true")
    ap.add_argument("--map", action="store_true", help="only the restore-map legs: the step launch and pipe() without / with a map")
    ap.add_argument("--apg", action="store_true", help="only the APG legs: the step launches and pipe() with APG off / on")
    args = ap.parse_args()
    from instantir_amd import schedulers as S, weights as W
    from instantir_amd.config import UNetConfig
    from instantir_amd.pipeline import InstantIRPipeline
    dev = torch.device("cuda:0")
    cfg = UNetConfig.tiny() if args.tiny else UNetConfig.sdxl()
    sd = W.synth_state_dict(W.unet_specs(cfg), 1234, device=dev)
    sda = W.synth_state_dict(W.aggregator_specs(cfg), 1235, device=dev)
    lora = W.synth_state_dict(W.lora_specs(cfg), 1236, device=dev)
    pipe = InstantIRPipeline(cfg, sd, scheduler=S.DDPMScheduler(), device=dev)
    pipe.aggregator.load_state_dict(sda)
    pipe.prepare_previewers(lora, lora_alpha=max(1, cfg.lora_rank // 8))
    lcm = S.LCMSingleStepScheduler.from_config(pipe.scheduler.config)
    g = torch.Generator().manual_seed(42)
    Hl = args.size // 8
    kw = dict(image=torch.randn(1, 4, Hl, Hl, generator=g) * 0.8,
              prompt_embeds=torch.randn(1, cfg.text_len, cfg.cross_attention_dim, generator=g),
              pooled_prompt_embeds=torch.randn(1, cfg.pooled_dim, generator=g),
              negative_prompt_embeds=torch.randn(1, cfg.text_len, cfg.cross_attention_dim, generator=g),
              negative_pooled_prompt_embeds=torch.randn(1, cfg.pooled_dim, generator=g),
              ip_adapter_image_embeds=[torch.randn(2, 1, cfg.resampler.seq_len, cfg.resampler.embedding_dim, generator=g)],
              init_noise=torch.randn(1, 4, Hl, Hl, generator=g), output_type="latent", previewer_scheduler=lcm, guidance_scale=7.0)
    base = pipe.scheduler.config
    scheds = {"ddpm": S.DDPMScheduler.from_config(base), "euler": S.EulerDiscreteScheduler.from_config(base),
              "dpmpp_2m": S.DPMSolverMultistepScheduler.from_config(base),
              "dpmpp_2m_karras": S.DPMSolverMultistepScheduler.from_config(base, use_karras_sigmas=True)}

    def call(name, n, **extra):
        pipe.scheduler = scheds[name]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = pipe(num_inference_steps=n, **kw, **extra).images
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert torch.isfinite(out).all(), name
        return dt

    if args.map:
        launch = map_launch_leg(args.size)
        rmap = torch.zeros(Hl, Hl)
        rmap[:, Hl // 2:] = 1.0
        rmap[: Hl // 2, : Hl // 2] = 0.4
        legs = {"no map": {}, "restore_map": {"restore_map": rmap}}
        res = {k: [] for k in legs}
        for r in range(args.pairs):
            for name, extra in legs.items():
                call("ddpm", 2, **extra)                # the loop cache holds one of the two forms: rebuild and capture, untimed
                dt = call("ddpm", args.steps, **extra)
                res[name].append(dt / args.steps * 1e3)
                print(f"round {r} ddpm {name}: {dt / args.steps * 1e3:.2f} ms/step (call {dt:.3f} s, {args.steps} steps)", flush=True)
        print(json.dumps({"size": args.size, "steps": args.steps, "step_launch_us_best": launch,
                          "ms_per_step_median": {k: round(statistics.median(v), 2) for k, v in res.items()},
                          "ms_per_step_all": {k: [round(x, 2) for x in v] for k, v in res.items()}}))
        return

    if args.apg:
        launch = {f"B={B}": apg_launch_leg(args.size, B) for B in (1, 8)}
        legs = {"apg off": None, "apg on": (0.0, 15.0, -0.5)}
        res = {k: [] for k in legs}
        for r in range(args.pairs):
            for name, par in legs.items():
                pipe.disable_apg() if par is None else pipe.enable_apg(*par)
                call("ddpm", 2)                         # the loop cache holds one of the two forms: rebuild and capture, untimed
                dt = call("ddpm", args.steps)
                res[name].append(dt / args.steps * 1e3)
                print(f"round {r} ddpm {name}: {dt / args.steps * 1e3:.2f} ms/step (call {dt:.3f} s, {args.steps} steps)", flush=True)
        pipe.disable_apg()
        print(json.dumps({"size": args.size, "steps": args.steps, "step_launch_us_best": launch,
                          "ms_per_step_median": {k: round(statistics.median(v), 2) for k, v in res.items()},
                          "ms_per_step_all": {k: [round(x, 2) for x in v] for k, v in res.items()}}))
        return

    # one untimed call per scheduler form (the loop cache holds one geometry x form: switching forms rebuilds and re-captures,
    # so every timed call below is preceded by an untimed call of the same form)
    res = {k: [] for k in ("ddpm", "euler", "dpmpp_2m")}
    for r in range(args.pairs):
        for name in ("ddpm", "euler", "dpmpp_2m"):
            call(name, 2)
            dt = call(name, args.steps)
            res[name].append(dt / args.steps * 1e3)
            print(f"round {r} {name}: {dt / args.steps * 1e3:.2f} ms/step (call {dt:.3f} s, {args.steps} steps)", flush=True)
    wall = {"ddpm_30": [], "dpmpp_2m_karras_20": []}
    for r in range(args.pairs):
        call("ddpm", 2)
        wall["ddpm_30"].append(call("ddpm", 30))
        call("dpmpp_2m_karras", 2)
        wall["dpmpp_2m_karras_20"].append(call("dpmpp_2m_karras", 20))
        print(f"round {r} wall: ddpm 30 steps {wall['ddpm_30'][-1]:.3f} s, dpmpp_2m karras 20 steps "
              f"{wall['dpmpp_2m_karras_20'][-1]:.3f} s", flush=True)
    print(json.dumps({"size": args.size, "steps": args.steps,
                      "ms_per_step_median": {k: round(statistics.median(v), 2) for k, v in res.items()},
                      "ms_per_step_all": {k: [round(x, 2) for x in v] for k, v in res.items()},
                      "wall_s_median": {k: round(statistics.median(v), 3) for k, v in wall.items()}}))


if __name__ == "__main__":
    main()
