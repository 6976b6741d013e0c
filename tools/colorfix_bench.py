"""Colour fix (color_fix: wavelet, adain) cost on one MI355X.

    python tools/colorfix_bench.py [--sizes 1024 2048] [--iters 50]

per size (B = 1, 3 channels), device events, best of two alternating windows of `--iters` calls: the HIP launches, the same
contract as plain torch ops on the device (wavelet: the textbook form, ten dilated depthwise conv2d + replicate pads;
adain: mean / var / normalise), and the byte floor from the shapes (content and style in, result out, plus the workspace
round trip) over 6.29 TB/s.

    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/colorfix_bench.py --kernels 50

launches only the HIP kernels, `--kernels` times per mode and size, for a per-kernel time table.

    python tools/colorfix_bench.py --call [--pairs 3] [--steps 30]

a 1024^2 `pipe(...)` (SDXL shapes, synthetic weights, pixel image in, 'pt' out) without and with color_fix="wavelet",
alternating pairs, medians."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

HBM_TBS = 6.29
LEVELS = (1, 2, 4, 8, 16)


def inputs(size, dev):
    g = torch.Generator().manual_seed(size)
    c = torch.rand(1, 3, size, size, generator=g).to(dev)
    s = (0.7 * F.avg_pool2d(c, 5, 1, 2) + 0.1 + 0.05 * torch.rand(1, 3, size, size, generator=g).to(dev)).clamp(0, 1)
    return c, s


def torch_wavelet(c, s, k):
    def decompose(x):
        high = torch.zeros_like(x)
        for r in LEVELS:
            low = F.conv2d(F.pad(x, (r, r, r, r), mode="replicate"), k, dilation=r, groups=3)
            high = high + (x - low)
            x = low
        return high, x
    return (decompose(c)[0] + decompose(s)[1]).clamp(0, 1)


def torch_adain(c, s):
    def stats(x):
        f = x.flatten(2)
        return f.mean(2)[..., None, None], (f.var(2) + 1e-5).sqrt()[..., None, None]
    mc, sc = stats(c)
    ms, ss = stats(s)
    return ((c - mc) / sc * ss + ms).clamp(0, 1)


def timed(fn, n):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def kernels(sizes, n, with_torch):
    from instantir_amd import lib, ops
    lib.load()
    dev = torch.device("cuda:0")
    k = (torch.tensor([[1.0, 2.0, 1.0], [2.0, 4.0, 2.0], [1.0, 2.0, 1.0]], device=dev) / 16).expand(3, 1, 3, 3).contiguous()
    for size in sizes:
        c, s = inputs(size, dev)
        out = torch.empty_like(c)
        ws = torch.empty(lib.load().iir_colorfix_workspace_bytes(1, 3, size, size), dtype=torch.uint8, device=dev)
        plane = 3 * size * size * 4
        # content and style in, result out, plus the workspace round trip (wavelet: one plane set out and back; adain: the slab table)
        floor = {"wavelet": 5 * plane, "adain": 3 * plane + 2 * 2 * 3 * 64 * 3 * 4}
        legs = {"wavelet": (lambda: ops.colorfix(c, s, "wavelet", out=out, ws=ws), lambda: torch_wavelet(c, s, k)),
                "adain": (lambda: ops.colorfix(c, s, "adain", out=out, ws=ws), lambda: torch_adain(c, s))}
        for mode, (hip, ref) in legs.items():
            if not with_torch:
                timed(hip, n)
                continue
            us = {"hip": 1e30, "torch": 1e30}
            for _ in range(2):
                us["hip"] = min(us["hip"], timed(hip, n))
                us["torch"] = min(us["torch"], timed(ref, n))
            fl = floor[mode] / (HBM_TBS * 1e12) * 1e6
            err = (out - ref()).abs().max().item()
            print(f"{mode:8s} {size}x{size} B=1: hip {us['hip']:.1f} us, torch ops {us['torch']:.1f} us ({us['torch'] / us['hip']:.1f}x), "
                  f"byte floor {floor[mode] / 1e6:.1f} MB = {fl:.1f} us ({100 * fl / us['hip']:.0f} % of it reached), "
                  f"max |hip - torch| {err:.1e}", flush=True)


def call(pairs, steps, size):
    from instantir_amd import lib, weights as W
    from instantir_amd.config import UNetConfig, VAEConfig
    from instantir_amd.pipeline import InstantIRPipeline
    from instantir_amd.schedulers import DDIMScheduler, LCMSingleStepScheduler
    from instantir_amd.vae import HipVAE
    lib.load()
    dev = torch.device("cuda:0")
    cfg, vc = UNetConfig.sdxl(), VAEConfig.sdxl()
    vae = HipVAE(vc, W.synth_state_dict(W.vae_decoder_specs(vc) + W.vae_encoder_specs(vc), 1237, device=dev), dev)
    pipe = InstantIRPipeline(cfg, W.synth_state_dict(W.unet_specs(cfg), 1234, device=dev), scheduler=DDIMScheduler(), vae=vae, device=dev)
    pipe.aggregator.load_state_dict(W.synth_state_dict(W.aggregator_specs(cfg), 1235, device=dev))
    pipe.prepare_previewers(W.synth_state_dict(W.lora_specs(cfg), 1236, device=dev), lora_alpha=cfg.lora_rank // 8)
    g = torch.Generator().manual_seed(42)
    kw = dict(image=torch.rand(1, 3, size, size, generator=g), prompt_embeds=torch.randn(1, cfg.text_len, cfg.cross_attention_dim, generator=g),
              pooled_prompt_embeds=torch.randn(1, cfg.pooled_dim, generator=g),
              ip_adapter_image_embeds=[torch.randn(2, 1, cfg.resampler.seq_len, cfg.resampler.embedding_dim, generator=g)],
              vae_noise=torch.randn(1, 4, size // 8, size // 8, generator=g), init_noise=torch.randn(1, 4, size // 8, size // 8, generator=g),
              num_inference_steps=steps, guidance_scale=7.0, previewer_scheduler=LCMSingleStepScheduler.from_config(pipe.scheduler.config),
              output_type="pt")

    def leg(mode):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = pipe(color_fix=mode, **kw).images
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    leg(None); leg("wavelet")                                          # set-up: arena sizing, graph capture
    res = {None: [], "wavelet": []}
    for p in range(pairs):
        for mode in (None, "wavelet"):
            ms, out = leg(mode)
            res[mode].append(ms)
            print(f"pair {p + 1} color_fix={mode} {ms:.1f} ms finite {bool(torch.isfinite(out).all().item())}", flush=True)
    a, b = statistics.median(res[None]), statistics.median(res["wavelet"])
    print(f"median pipe(...) {size}^2, {steps} steps, cfg 7: none {a:.1f} ms, wavelet {b:.1f} ms ({b - a:+.2f} ms, {100 * (b - a) / a:+.2f} %)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 2048])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--kernels", type=int, default=0, help="only launch the HIP kernels this many times (for rocprofv3)")
    ap.add_argument("--call", action="store_true")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=30)
    args = ap.parse_args()
    if args.call:
        return call(args.pairs, args.steps, 1024)
    kernels(args.sizes, args.kernels or args.iters, with_torch=not args.kernels)


if __name__ == "__main__":
    main()
