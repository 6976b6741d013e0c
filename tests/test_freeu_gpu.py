"""GPU: FreeU (module/min_sdxl.py:22-77, applied before the up blocks' concats, module/unet/unet_2d_ZeroSFT_blocks.py:2600-2627,
2748-2775) through the HIP kernels of csrc/freeu.hip and the pipeline's `enable_freeu`.

The oracle is the fp32 torch.fft restatement in tests/test_freeu_cpu.py, which is pinned to the reference's own outputs
(tests/golden/freeu.npz).  The whole-loop tests FreeU the CPU oracle by swapping `oracle.nets.up_block` for a wrapper that
applies that restatement by `up_blocks.{i}` index (oracle/ itself is not edited)."""
import functools

import pytest
import torch
import torch.nn.functional as F

import loop_ref as lr
from loop_ref import dev, env  # noqa: F401  (fixtures)
from test_freeu_cpu import apply_freeu, fourier_filter

pytestmark = pytest.mark.gpu

SDXL = (0.9, 0.2, 1.3, 1.4)      # s1, s2, b1, b2: diffusers' SDXL values
BAR = 50.0


def _ulp16(a):
    """one fp16 ulp at |a| (subnormal spacing below 2^-14)"""
    e = torch.floor(torch.log2(a.abs().clamp_min(2.0 ** -14)))
    return torch.pow(2.0, e - 10)


def _case(dev, R, H, W, cx, cs, mode, b, s, seed=0, off=8, tail=16):
    """One stats + concat into a NaN-filled (rows, off + cx + cs + tail) buffer.  Returns (cat, inputs)."""
    from instantir_amd import ops
    g = torch.Generator().manual_seed(seed + 7 * H + W + cx + cs)
    rows = R * H * W
    rnd = lambda *sh, scale=1.0: (torch.randn(*sh, generator=g) * scale).half().to(dev)
    x, sk = rnd(rows, cx, scale=1.5), rnd(rows, cs, scale=1.2)
    add = rnd(rows, cs, scale=0.5) if mode != "plain" else None
    mid = rnd(rows, cx, scale=0.5) if mode == "add+mid" else None
    scale = torch.tensor([0.7, 1.25, 0.4][:R], dtype=torch.float32, device=dev) if mode != "plain" else None
    cat = torch.full((rows, off + cx + cs + tail), float("nan"), dtype=torch.half, device=dev)
    parts = torch.empty(ops.freeu_partials_floats(rows, H, W, cs), dtype=torch.float32, device=dev)
    ops.freeu_stats(sk, parts, H, W, add=add, add_scale=scale)
    ops.freeu_concat(x, sk, cat, parts, H, W, b, s, dst_off=off, mid_add=mid, add=add, add_scale=scale)
    torch.cuda.synchronize()
    return cat, dict(x=x, sk=sk, add=add, mid=mid, scale=scale, off=off)


def _want(inp, R, H, W, b, s):
    """fp32: t = v + add * scale (same op order as the kernel), hidden half times b, fourier_filter(skip) by torch.fft."""
    x, sk = inp["x"].float().cpu(), inp["sk"].float().cpu()
    HW = H * W
    if inp["scale"] is not None:
        sc = inp["scale"].cpu().repeat_interleave(HW)[:, None]
        if inp["mid"] is not None:
            x = x + inp["mid"].float().cpu() * sc
        if inp["add"] is not None:
            sk = sk + inp["add"].float().cpu() * sc
    cx, cs = x.shape[1], sk.shape[1]
    hid = x.clone()
    hid[:, :cx // 2] = hid[:, :cx // 2] * b
    skn = sk.view(R, H, W, cs).permute(0, 3, 1, 2)
    filt = fourier_filter(skn, s).permute(0, 2, 3, 1).reshape(R * HW, cs)
    return hid, filt


TABLE = [(32, 32, 1280, 1280), (32, 32, 1280, 640), (64, 64, 1280, 640), (64, 64, 640, 640), (64, 64, 640, 320)]
EXTRA = [(24, 32, 1280, 640), (48, 64, 640, 320), (4, 4, 256, 256), (4, 4, 256, 128), (8, 8, 256, 128), (8, 8, 128, 64),
         (5, 7, 64, 40), (1, 4, 16, 8), (3, 1, 8, 8), (1, 1, 8, 8)]


@pytest.mark.parametrize("H,W,cx,cs", TABLE + EXTRA)
@pytest.mark.parametrize("mode", ["plain", "add", "add+mid"])
def test_kernels_match_fft_freeu(dev, H, W, cx, cs, mode):
    """Kernel pair vs the fp32 torch.fft FreeU, R = 2.  Bound: the hidden half is the fp16 rounding of the same fp32 product
    (bit-exact); the filtered skip is within ONE fp16 ulp of the fp32 FFT result (half an ulp of rounding, plus fp32
    evaluation-order differences that can move a value across a rounding boundary) + 1e-5.  Columns of the wider buffer
    outside [off, off + cx + cs) keep their NaNs."""
    R = 2
    for idx, (b, s) in enumerate([(SDXL[2], SDXL[0]), (SDXL[3], SDXL[1])]):
        cat, inp = _case(dev, R, H, W, cx, cs, mode, b, s, seed=idx)
        off = inp["off"]
        hid, filt = _want(inp, R, H, W, b, s)
        got_h = cat[:, off:off + cx].cpu()
        got_s = cat[:, off + cx:off + cx + cs].cpu().float()
        assert torch.equal(got_h, hid.half()), f"hidden half differs ({(got_h.float() - hid).abs().max().item()})"
        err = (got_s - filt).abs()
        lim = _ulp16(filt) + 1e-5
        assert torch.isfinite(got_s).all() and bool((err <= lim).all()), \
            f"skip: max err {err.max().item():.3g}, worst ratio {(err / lim).max().item():.3g}"
        assert torch.isnan(cat[:, :off]).all() and torch.isnan(cat[:, off + cx + cs:]).all(), "wrote outside the concat columns"


@pytest.mark.parametrize("H,W,cx,cs", TABLE + [(24, 32, 1280, 640), (4, 4, 256, 128), (5, 7, 64, 40)])
def test_identity_factors_equal_copy_add_pair(dev, H, W, cx, cs):
    """s = 1, b = 1: the concat is bit-identical to the two iir_copy_add_f16 launches it replaces (add + per-row scale on both)."""
    from instantir_amd import ops
    R = 2
    cat, inp = _case(dev, R, H, W, cx, cs, "add+mid", 1.0, 1.0, off=0, tail=0)
    ref = torch.empty_like(cat)
    ops.copy_add(inp["x"], ref, 0, add=inp["mid"], add_scale=inp["scale"], rows_per_scale=H * W)
    ops.copy_add(inp["sk"], ref, cx, add=inp["add"], add_scale=inp["scale"], rows_per_scale=H * W)
    torch.cuda.synchronize()
    assert torch.equal(cat.view(torch.int16), ref.view(torch.int16))


def test_kernels_reproducible_beside_a_busy_stream(dev):
    """Race screen: the two launches give bit-identical output while a second stream runs GEMM + attention + conv."""
    from instantir_amd import ops
    g = torch.Generator().manual_seed(5)
    rnd = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).half().to(dev)
    side = torch.cuda.Stream()
    nx, nw, no = rnd(4096, 1280), rnd(2560, 1280, scale=0.03), torch.empty(4096, 2560, dtype=torch.half, device=dev)
    nq, nvt, nao = rnd(2 * 2048, 2 * 640), rnd(640, 2 * 2048), torch.empty(2 * 2048, 640, dtype=torch.half, device=dev)
    ncx, ncw, nco = rnd(2, 64, 64, 640), rnd(640, 3, 3, 640, scale=0.02), torch.empty(2 * 64 * 64, 640, dtype=torch.half, device=dev)

    def noise():
        with torch.cuda.stream(side):
            for _ in range(3):
                ops.gemm(nx, nw, no)
                ops.attention(nq[:, :640], nao, [(nq[:, 640:], 2048, nvt, 2048, 2048)], 2, 10, 2048)
                ops.conv2d(ncx, ncw, nco)

    for (H, W, cx, cs) in [(32, 32, 1280, 1280), (64, 64, 640, 320)]:
        rows = 2 * H * W
        x, sk, add, mid = rnd(rows, cx), rnd(rows, cs), rnd(rows, cs, scale=0.5), rnd(rows, cx, scale=0.5)
        sc = torch.tensor([0.8, 1.1], device=dev)
        first = None
        for it in range(8):
            parts = torch.zeros(ops.freeu_partials_floats(rows, H, W, cs), dtype=torch.float32, device=dev)
            cat = torch.zeros(rows, cx + cs, dtype=torch.half, device=dev)
            noise()
            ops.freeu_stats(sk, parts, H, W, add=add, add_scale=sc)
            noise()
            ops.freeu_concat(x, sk, cat, parts, H, W, 1.3, 0.9, mid_add=mid, add=add, add_scale=sc)
            torch.cuda.synchronize()
            bits = torch.cat([parts.view(torch.int32).flatten().long(), cat.view(torch.int16).flatten().long()])
            if first is None:
                first = bits
            else:
                assert torch.equal(bits, first), f"{H}x{W}: launch {it} differs from launch 0"


# ---- through the pipeline -----------------------------------------------------------------------------------------------
psnr = lr.psnr_by_caller("freeu")


def freeu_up_block(factors):
    """oracle.nets.up_block with apply_freeu on each (hidden, skip) pair before the concat, resolution_idx = i of up_blocks.i."""
    from oracle import nets

    def up_block(P, path, x, skips, emb, ctx, ip_tokens, depth, heads, groups, has_up, lora=None):
        idx = int(path.rsplit(".", 1)[1])
        skips = list(skips)
        for j in range(len(skips)):
            h, sk = apply_freeu(idx, x, skips.pop(), factors)
            x = torch.cat([h, sk], dim=1)
            x = nets.resnet(P, f"{path}.resnets.{j}", x, emb, groups, lora)
            if depth > 0:
                x = nets.transformer2d(P, f"{path}.attentions.{j}", x, depth, ctx, ip_tokens, emb, heads, groups, lora)
        if has_up:
            x = F.interpolate(x, scale_factor=2.0, mode="nearest")
            x = nets.conv2d(P, f"{path}.upsamplers.0.conv", x, lora=lora)
        return x
    return up_block


LOOP = dict(guidance_scale=7.0, **lr.LOOP)
_call = functools.partial(lr.call, **LOOP)


def test_identity_factors_bit_identical_to_off(env):
    """enable_freeu(1, 1, 1, 1) is ON (all factors truthy) and runs the FreeU kernels, yet gives the FreeU-off latents bit for
    bit: hipGraphs, two streams, all loop phases."""
    cfg, sd, sda, lora, inp = env
    pipe = lr.pipe(env)
    assert pipe.use_graphs and pipe.overlap_streams
    off = _call(pipe, inp)
    pipe2 = lr.pipe(env)
    pipe2.enable_freeu(1, 1, 1, 1)
    on = _call(pipe2, inp)
    assert pipe2._unet.freeu == (1.0, 1.0, 1.0, 1.0) and pipe2._unet_prev.freeu == (1.0, 1.0, 1.0, 1.0)
    assert torch.equal(on, off)


def test_loop_matches_freeu_oracle(env, monkeypatch):
    """DDIM + CFG, agg / preview / unet phases, s1=0.9 s2=0.2 b1=1.3 b2=1.4 on the main and the previewer UNet: >= 50 dB against
    the FreeU'd oracle loop, and clearly (>= 6 dB) further from the plain oracle."""
    from oracle import nets
    cfg, sd, sda, lora, inp = env
    plain = lr.denoise(env, sampler="ddim", **LOOP)
    monkeypatch.setattr(nets, "up_block", freeu_up_block(SDXL))
    want = lr.denoise(env, sampler="ddim", **LOOP)
    pipe = lr.pipe(env)
    pipe.enable_freeu(*SDXL)
    got = _call(pipe, inp)
    p, p_plain = psnr(got, want), psnr(got, plain)
    assert torch.isfinite(got).all() and p >= BAR, p
    assert p_plain < p - 6, (p, p_plain)


def test_restore_single_step_with_freeu(env, monkeypatch):
    """restore_single_step (one previewer-LoRA pass + LCM step) with FreeU vs the FreeU'd oracle pass."""
    from oracle import nets, sched
    cfg, sd, sda, lora, inp = env
    pipe = lr.pipe(env)
    pipe.unet.enable_freeu(*SDXL)            # the unet-level switch: same state
    feats = inp["img"][1:]
    got = pipe.restore_single_step(inp["lq"], inp["pe"], inp["pooled"], ip_adapter_image_embeds=[feats], init_noise=inp["init_noise"],
                                   output_type="latent").images.float().cpu()
    P, _, L = lr.params(env)
    acp = sched.make_alphas_cumprod()
    B = inp["B"]
    x = sched.add_noise(acp, inp["lq"], inp["init_noise"], [999] * B)
    tid = torch.tensor([[128.0, 128, 0, 0, 128, 128]]).repeat(B, 1)
    ip = nets.image_projection(P, [feats], cfg.resampler, L)[0]
    plain = sched.lcm_step(acp, nets.unet_forward(P, cfg, x, 999, inp["pe"], inp["pooled"], tid, ip, lora=L), 999, x)
    monkeypatch.setattr(nets, "up_block", freeu_up_block(SDXL))
    want = sched.lcm_step(acp, nets.unet_forward(P, cfg, x, 999, inp["pe"], inp["pooled"], tid, ip, lora=L), 999, x)
    p, p_plain = psnr(got, want), psnr(got, plain)
    assert torch.isfinite(got).all() and p >= BAR and p_plain < p - 6, (p, p_plain)


def test_toggling_between_calls_replays_the_right_graphs(env):
    """off -> on -> off -> on (changed factor) on ONE pipeline (loop cache, captured graphs): each call equals a fresh pipeline
    with that setting, bit for bit."""
    cfg, sd, sda, lora, inp = env
    settings = [None, SDXL, None, (0.9, 0.5, 1.3, 1.4)]
    pipe = lr.pipe(env)
    for f in settings:
        if f is None:
            pipe.disable_freeu()
        else:
            pipe.enable_freeu(*f)
        got = _call(pipe, inp)
        fresh = lr.pipe(env)
        if f is not None:
            fresh.enable_freeu(*f)
        assert torch.equal(got, _call(fresh, inp)), f
    assert not torch.equal(got, _call(lr.pipe(env), inp))


def test_config1_geometry_one_step_with_freeu(dev, monkeypatch):
    """configs[1]'s geometry (1024^2, cfg 7, B = 1: the 32x32 / 64x64 concats of the table) for one step at t = 501 with FreeU
    on, against the FreeU'd CPU oracle (as tests/test_fullsize_gpu.py does for the plain step); two calls bit-identical."""
    import os
    from instantir_amd import weights as W
    from instantir_amd.config import UNetConfig
    from instantir_amd.pipeline import InstantIRPipeline
    from instantir_amd.schedulers import DDPMScheduler, LCMSingleStepScheduler
    from oracle import nets, pipeline as OP
    cfg = UNetConfig.sdxl()
    sd = W.synth_state_dict(W.unet_specs(cfg), 1234, device=dev)
    sda = W.synth_state_dict(W.aggregator_specs(cfg), 1235, device=dev)
    lora = W.synth_state_dict(W.lora_specs(cfg), 1236, device=dev)
    g = torch.Generator().manual_seed(42)
    B, H = 1, 128
    lq = torch.randn(B, 4, H, H, generator=g) * 0.8
    pe = torch.randn(B, 77, 2048, generator=g).half().float()
    pooled = torch.randn(B, 1280, generator=g).half().float()
    feats = torch.randn(2, B, 257, 1024, generator=g).half().float()
    npe = torch.randn(B, 77, 2048, generator=g).half().float()
    npooled = torch.randn(B, 1280, generator=g).half().float()
    noise = torch.randn(B, 4, H, H, generator=g)
    sn = [torch.randn(B, 4, H, H, generator=g)]
    pipe = InstantIRPipeline(cfg, sd, scheduler=DDPMScheduler(), device=dev)
    pipe.aggregator.load_state_dict(sda)
    pipe.prepare_previewers(lora, lora_alpha=8)
    pipe.enable_freeu(*SDXL)
    kw = dict(image=lq, prompt_embeds=pe, pooled_prompt_embeds=pooled, negative_prompt_embeds=npe, negative_pooled_prompt_embeds=npooled,
              ip_adapter_image_embeds=[feats], output_type="latent", num_inference_steps=1, guidance_scale=7.0, init_noise=noise,
              timesteps=[501], step_noises=sn, previewer_scheduler=LCMSingleStepScheduler.from_config(pipe.scheduler.config))
    got = pipe(**kw).images.float().cpu()
    again = pipe(**kw).images.float().cpu()
    assert torch.isfinite(got).all() and torch.equal(got, again)
    n = len(os.sched_getaffinity(0))
    torch.set_num_threads(max(1, min(n, 16)))
    P = {k: v.float().cpu() for k, v in sd.items()}
    PA = {k: v.float().cpu() for k, v in sda.items()}
    L = {k: v.float().cpu() for k, v in lora.items()}
    L["scaling"] = 8 / cfg.lora_rank
    del sd, sda, lora, pipe
    torch.cuda.empty_cache()
    monkeypatch.setattr(nets, "up_block", freeu_up_block(SDXL))
    with torch.no_grad():
        want = OP.denoise(P, PA, L, cfg, lq, pe, pooled, feats, negative_prompt_embeds=npe, negative_pooled=npooled, init_noise=noise,
                          num_inference_steps=1, guidance_scale=7.0, sampler="ddpm", timesteps=[501], step_noises=sn)
    p = psnr(got, want)
    print(f"configs[1] geometry, one step with FreeU: latent PSNR vs CPU fp32 oracle {p:.1f} dB")
    assert p >= BAR, p
