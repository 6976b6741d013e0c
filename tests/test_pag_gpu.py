"""GPU: perturbed-attention guidance (PAG, Ahn et al. 2024) -- the identity rows of iir_attention_d64_ident_f16, the PAG forms
of the step launches against fp32 torch, and the denoising loop against a PAG'd fp32 CPU oracle.

The oracle gets PAG without editing oracle/nets.py (tests/loop_ref.py): `oracle.nets.attn_self` is swapped for a wrapper that returns
to_out(to_v(x)) for the perturbed rows of the selected layers, the oracle loops' `main_unet` hook runs the main UNet on [uncond;]
cond; perturbed rows, each perturbed row a copy of its cond row's inputs and Aggregator residuals, and their `guide` hook adds
s_t (c - p)."""
import functools
import os

import numpy as np
import pytest
import torch

import loop_ref as lr
from loop_ref import dev, env, pag_oracle_attn  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

BAR = 60.0


psnr = lr.psnr_by_caller("pag")


# ---- identity attention ---------------------------------------------------------------------------------------------------
def _attn_case(dev, T, heads, batch, seed=0):
    """q|k in one (batch*T, 2C) buffer and V^T as (C, batch*vbs), as the fused q|k|v GEMM leaves them (vbs = T rounded up to 8,
    pad columns zero)."""
    g = torch.Generator().manual_seed(seed + T + heads + batch)
    C = heads * 64
    vbs = (T + 7) // 8 * 8
    qk = (torch.randn(batch * T, 2 * C, generator=g) * 0.5).half().to(dev)
    vt = torch.zeros(C, batch * vbs, dtype=torch.half)
    for b in range(batch):
        vt[:, b * vbs:b * vbs + T] = torch.randn(C, T, generator=g).half()
    return qk, vt.to(dev), C, vbs


def _attn(qk, vt, C, vbs, T, heads, batch, ident_from, dev):
    from instantir_amd import ops
    o = torch.full((batch * T, C), float("nan"), dtype=torch.half, device=dev)
    ops.attention(qk[:, :C], o, [(qk[:, C:], T, vt, vbs, T)], batch, heads, T, q_prescaled=True, ident_from=ident_from)
    return o


SHAPES = [(4096, 10, 3, 2), (1024, 20, 3, 2), (4096, 10, 2, 1), (1024, 20, 2, 1),      # the step's shapes (cfg / no cfg)
          (333, 2, 3, 1), (1023, 5, 2, 1), (77, 4, 3, 2), (64, 3, 2, 1), (200, 2, 4, 2), (5, 1, 2, 1)]   # odd T, the short-KV form


@pytest.mark.parametrize("T,heads,batch,ident_from", SHAPES)
def test_identity_rows_equal_v_and_other_rows_equal_plain(dev, T, heads, batch, ident_from):
    qk, vt, C, vbs = _attn_case(dev, T, heads, batch)
    got = _attn(qk, vt, C, vbs, T, heads, batch, ident_from, dev)
    plain = _attn(qk, vt, C, vbs, T, heads, batch, 0, dev)
    torch.cuda.synchronize()
    n = ident_from * T
    assert torch.equal(got[:n].view(torch.int16), plain[:n].view(torch.int16))       # attending rows: bit-identical
    v = torch.cat([vt[:, b * vbs:b * vbs + T].t() for b in range(ident_from, batch)])
    assert torch.equal(got[n:].view(torch.int16), v.view(torch.int16))               # identity rows: V, bit for bit


def test_identity_attention_reproducible_beside_a_busy_stream(dev):
    """Race screen: two launches each give bit-identical output while a second stream runs GEMM + attention + conv."""
    from instantir_amd import ops
    g = torch.Generator().manual_seed(5)
    rnd = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).half().to(dev)
    side = torch.cuda.Stream()
    nx, nw, no = rnd(4096, 1280), rnd(2560, 1280, scale=0.03), torch.empty(4096, 2560, dtype=torch.half, device=dev)
    ncx, ncw, nco = rnd(2, 64, 64, 640), rnd(640, 3, 3, 640, scale=0.02), torch.empty(2 * 64 * 64, 640, dtype=torch.half, device=dev)
    for (T, heads, batch, f) in [(4096, 10, 3, 2), (1024, 20, 3, 2)]:
        qk, vt, C, vbs = _attn_case(dev, T, heads, batch, seed=3)
        outs = []
        for _ in range(2):
            with torch.cuda.stream(side):
                for _ in range(3):
                    ops.gemm(nx, nw, no)
                    ops.attention(qk[:, :C], torch.empty(batch * T, C, dtype=torch.half, device=dev), [(qk[:, C:], T, vt, vbs, T)],
                                  batch, heads, T, q_prescaled=True)
                    ops.conv2d(ncx, ncw, nco)
            outs.append(_attn(qk, vt, C, vbs, T, heads, batch, f, dev))
            torch.cuda.synchronize()
        assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))


# ---- PAG step launches ------------------------------------------------------------------------------------------------------
def _pag_eps(e, B, cfg, g, s, fac=None):
    """fp32 guided eps with the PAG term, times the rescale factor `fac` when given, in the kernels' op order; and the fp64
    rescale_noise_cfg ratio std(c) / std(eps) per image."""
    g, s = torch.tensor(g, dtype=torch.float32), torch.tensor(s, dtype=torch.float32)
    if cfg:
        u, c, p = e[:B], e[B:2 * B], e[2 * B:3 * B]
        out = u + g * (c - u)
        out = out + s * (c - p)
        ratio = c.double().std(dim=(1, 2, 3)) / out.double().std(dim=(1, 2, 3))
        if fac is not None:
            out = out * fac.view(B, 1, 1, 1)
        return out, ratio
    c, p = e[:B], e[B:2 * B]
    return c + s * (c - p), None


@pytest.mark.parametrize("form", ["linear", "hist"])
@pytest.mark.parametrize("cfg,phi", [(True, 0.0), (False, 0.0), (True, 0.7)])
@pytest.mark.parametrize("B,H,W", [(1, 128, 128), (2, 5, 7)])
def test_pag_step_matches_fp32(dev, form, cfg, phi, B, H, W):
    from instantir_amd import ops
    g = torch.Generator().manual_seed(B * 100 + H + int(cfg) + int(phi * 10))
    C, lde, HW = 4, 8, H * W
    R = B * (3 if cfg else 2)
    eps16 = torch.randn(R * HW, lde, generator=g).half()
    x = torch.randn(B, C, H, W, generator=g) * 3
    m = torch.randn(B, C, H, W, generator=g)
    nz = torch.randn(B, C, H, W, generator=g)
    coef = [6.5, 0.93, 0.37, 0.41, 0.98, 0.12, 0.07, -0.031 if form == "hist" else 0.0]
    s = 2.75
    ps = torch.tensor([s], dtype=torch.float32, device=dev)
    cd = torch.tensor(coef).to(dev)
    fac = None
    if phi > 0:
        fac = ops.cfg_rescale_factor(eps16.to(dev), B, cd, x.to(dev), phi, torch.empty(B, device=dev), pag_scale=ps)
    prev, x0 = torch.empty(B, C, H, W, device=dev), torch.empty(B, C, H, W, device=dev)
    if form == "hist":
        hist = m.clone().to(dev)
        ops.sched_step_hist(eps16.to(dev), B, cd, x.to(dev), hist, prev, noise=nz.to(dev), cfg=cfg, x0_out=x0, eps_factor=fac,
                            pag_scale=ps)
    else:
        ops.sched_step(eps16.to(dev), B, cd, x.to(dev), prev, noise=nz.to(dev), cfg=cfg, x0_out=x0, eps_factor=fac, pag_scale=ps)
    torch.cuda.synchronize()
    e = eps16.float()[:, :C].reshape(R, H, W, C).permute(0, 3, 1, 2)
    eg, ratio = _pag_eps(e, B, cfg, coef[0], s, None if fac is None else fac.cpu())
    if fac is not None:
        # the factor on its own (a one-ulp change of it moves cancelling outputs by many of their ulps, so the step below uses
        # the kernel's factor, as tests/test_sigma_schedulers_gpu.py does)
        want_fac = (phi * ratio + (1 - phi)).float()
        assert ((fac.cpu().double() - want_fac.double()).abs() / want_fac.double()).max().item() <= 2.0 ** -21
    want, want_x0 = lr.ref_step(eg, x, coef, m if form == "hist" else None, nz)
    assert lr.ulps(prev.cpu(), want) <= 4 and lr.ulps(x0.cpu(), want_x0) <= 4


@pytest.mark.parametrize("form", ["linear", "hist"])
@pytest.mark.parametrize("cfg", [True, False])
def test_pag_step_with_zero_scale_is_bit_identical_to_plain(dev, form, cfg):
    """s_t = 0: the PAG forms give the plain launches' bits (rescale factor included), whatever the perturbed rows hold."""
    from instantir_amd import ops
    g = torch.Generator().manual_seed(17)
    B, C, H, W, lde = 2, 4, 32, 24, 8
    HW = H * W
    Rp, R = B * (3 if cfg else 2), B * (2 if cfg else 1)
    eps = torch.randn(Rp * HW, lde, generator=g).half().to(dev)
    x = (torch.randn(B, C, H, W, generator=g) * 3).to(dev)
    nz = torch.randn(B, C, H, W, generator=g).to(dev)
    m = torch.randn(B, C, H, W, generator=g).to(dev)
    cd = torch.tensor([6.5, 0.93, 0.37, 0.41, 0.98, 0.12, 0.07, -0.031 if form == "hist" else 0.0]).to(dev)
    zero = torch.zeros(1, device=dev)
    outs = []
    for ps in (zero, None):
        fac = ops.cfg_rescale_factor(eps, B, cd, x, 0.7, torch.empty(B, device=dev), pag_scale=ps) if cfg else None
        prev, x0 = torch.empty_like(x), torch.empty_like(x)
        if form == "hist":
            hist = m.clone()
            ops.sched_step_hist(eps if ps is not None else eps[:R * HW], B, cd, x, hist, prev, noise=nz, cfg=cfg, x0_out=x0,
                                eps_factor=fac, pag_scale=ps)
        else:
            ops.sched_step(eps if ps is not None else eps[:R * HW], B, cd, x, prev, noise=nz, cfg=cfg, x0_out=x0, eps_factor=fac,
                           pag_scale=ps)
        outs.append((prev, x0, fac))
    torch.cuda.synchronize()
    for a, b in zip(outs[0], outs[1]):
        if a is not None:
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_copy_segments(dev):
    from instantir_amd import ops
    a = torch.randn(3 * 4096, 320, device=dev).half()
    b = torch.randn(3 * 64, 1280, device=dev).half()
    a0, b0 = a.clone(), b.clone()
    tab = ops.segment_job_table([(a[4096:8192], a[8192:]), (b[64:128], b[128:])], dev)
    ops.copy_segments(*tab)
    torch.cuda.synchronize()
    assert torch.equal(a[:8192], a0[:8192]) and torch.equal(a[8192:], a0[4096:8192])
    assert torch.equal(b[:128], b0[:128]) and torch.equal(b[128:], b0[64:128])


# ---- the denoising loop ----------------------------------------------------------------------------------------------------
LOOP = lr.LOOP
_call = functools.partial(lr.call, **LOOP)


CASES = {
    "cfg7_mid": (dict(guidance_scale=7.0, pag_scale=3.0), "mid", {}),
    "cfg1_up0": (dict(guidance_scale=1.0, pag_scale=3.0), "up_blocks.0", {}),
    "rescale": (dict(guidance_scale=7.0, pag_scale=2.0, guidance_rescale=0.7), ["mid", "down_blocks.2"], {}),
    "adastep": (dict(guidance_scale=5.0, pag_scale=3.0, pag_adaptive_scale=0.002), "mid", dict(adastep_restore=True)),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_loop_matches_pag_oracle(env, pag_oracle_attn, case):
    """PAG through every phase (Aggregator-only head, previewed middle, creative tail): >= 60 dB against the PAG'd oracle and
    at least 6 dB closer to it than to the plain oracle."""
    from instantir_amd import pag
    call_kw, layers, extra = CASES[case]
    cfg = env[0]
    paths = pag.select(layers, pag.attn1_paths(cfg))
    okw = dict(scale=call_kw["pag_scale"], adaptive=call_kw.get("pag_adaptive_scale", 0.0))
    g, phi = call_kw["guidance_scale"], call_kw.get("guidance_rescale", 0.0)
    want = lr.denoise(env, g, main_unet=lr.pag_unet(paths, env[4]["B"]), guide=lr.perturbed(g, **okw), guidance_rescale=phi,
                      **LOOP, **extra)
    plain = lr.denoise(env, g, guidance_rescale=phi, **LOOP, **extra)
    pipe = lr.pipe(env)
    pipe.enable_pag(layers)
    got = _call(pipe, env[4], **call_kw, **extra)
    p, p_plain = psnr(got, want), psnr(got, plain)
    print(f"{case}: latent PSNR vs PAG'd oracle {p:.1f} dB, vs plain oracle {p_plain:.1f} dB")
    assert torch.isfinite(got).all() and p >= BAR, p
    assert p_plain < p - 6, (p, p_plain)


def test_dpmpp_2m_karras_adaptive_matches_pag_oracle(env, pag_oracle_attn):
    """DPM++ 2M Karras with pag_adaptive_scale > 0 (fractional timesteps reach s_t), against the sigma-scheduler oracle loop with
    the same two hooks."""
    from instantir_amd import pag
    cfg, inp = env[0], env[4]
    paths = pag.select("mid", pag.attn1_paths(cfg))
    g, s, a = 5.0, 3.0, 0.002
    plain = lr.sigma_denoise(env, "dpm", 8, guidance_scale=g, karras=True, **lr.PHASES)
    want = lr.sigma_denoise(env, "dpm", 8, guidance_scale=g, karras=True, main_unet=lr.pag_unet(paths, inp["B"]),
                            guide=lr.perturbed(g, s, a), **lr.PHASES)
    pipe = lr.pipe(env, lr.sigma_sched("dpm", karras=True))
    pipe.enable_pag("mid")
    got = _call(pipe, inp, guidance_scale=g, pag_scale=s, pag_adaptive_scale=a, num_inference_steps=8, **lr.PHASES)
    p, p_plain = psnr(got, want), psnr(got, plain)
    print(f"dpmpp_2m karras adaptive: latent PSNR vs PAG'd oracle {p:.1f} dB, vs plain oracle {p_plain:.1f} dB")
    assert torch.isfinite(got).all() and p >= BAR, p
    assert p_plain < p - 6, (p, p_plain)


def test_disabled_and_zero_scale_bit_identical_to_never_enabled(env):
    inp = env[4]
    base = _call(lr.pipe(env), inp)
    p = lr.pipe(env)
    p.enable_pag("mid")
    p.disable_pag()
    assert torch.equal(_call(p, inp), base)
    p2 = lr.pipe(env)
    p2.enable_pag(["mid", "up_blocks.0"])
    assert torch.equal(_call(p2, inp, pag_scale=0.0), base)
    assert p2._unet.pag is None                                  # scale 0: the plain launches ran


def test_toggling_between_calls_replays_the_right_graphs(env):
    """off -> mid -> off -> mid+up_blocks.0 -> mid (other scale) on ONE pipeline: each call equals a fresh pipeline with that
    setting, bit for bit."""
    inp = env[4]
    settings = [None, ("mid", 3.0), None, (["mid", "up_blocks.0"], 3.0), ("mid", 1.5)]
    pipe = lr.pipe(env)
    outs = []
    for st in settings:
        if st is None:
            pipe.disable_pag()
            got = _call(pipe, inp)
            fresh = _call(lr.pipe(env), inp)
        else:
            pipe.enable_pag(st[0])
            got = _call(pipe, inp, pag_scale=st[1])
            f = lr.pipe(env)
            f.enable_pag(st[0])
            fresh = _call(f, inp, pag_scale=st[1])
        assert torch.equal(got, fresh), st
        outs.append(got)
    assert not torch.equal(outs[0], outs[1]) and not torch.equal(outs[1], outs[3]) and not torch.equal(outs[1], outs[4])


def test_graphs_on_off_repeat_calls_and_callback_bit_identical(env):
    inp = env[4]
    pipe = lr.pipe(env)
    pipe.enable_pag("mid")
    a = _call(pipe, inp, pag_adaptive_scale=0.001)
    b = _call(pipe, inp, pag_adaptive_scale=0.001)
    pipe.use_graphs = False
    c = _call(pipe, inp, pag_adaptive_scale=0.001)
    pipe.use_graphs, pipe.overlap_streams = True, False
    d = _call(pipe, inp, pag_adaptive_scale=0.001)
    assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, d)
    seen = []

    def cb(p, i, t, kw):          # prompt_embeds seen by the callback: the 2B-row [neg; pos] context; returning it rebuilds
        seen.append(tuple(kw["prompt_embeds"].shape))
        return {"prompt_embeds": kw["prompt_embeds"].clone()} if i == 3 else {}
    pipe.overlap_streams = True
    e = _call(pipe, inp, pag_adaptive_scale=0.001, callback_on_step_end=cb, callback_on_step_end_tensor_inputs=["latents", "prompt_embeds"])
    assert torch.equal(a, e) and set(seen) == {(2 * inp["B"], env[0].text_len, env[0].cross_attention_dim)}


def test_composes_with_freeu_reference_latents_and_images_per_prompt(env):
    """FreeU, reference_latents, num_images_per_prompt and save_preview_row run with PAG (finite, deterministic, and PAG
    changes the result)."""
    cfg, inp = env[0], env[4]
    one = {k: (v[:1] if k in ("lq", "pe", "pooled", "npe", "npooled", "init_noise") else v) for k, v in inp.items()}
    one["img"] = inp["img"][:, :1]
    one["B"] = 1
    ref = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(3)) * 0.5       # one per image of the batch
    kw = dict(reference_latents=ref, num_images_per_prompt=2, save_preview_row=True, return_dict=False)

    def run(pag_on):
        from instantir_amd.schedulers import LCMSingleStepScheduler
        p = lr.pipe(env)
        p.enable_freeu(0.9, 0.2, 1.3, 1.4)
        extra = {}
        if pag_on:
            p.enable_pag(["mid", "up_blocks.1"])
            extra = dict(pag_scale=3.0)
        out, row = p(image=one["lq"], prompt_embeds=one["pe"], pooled_prompt_embeds=one["pooled"], negative_prompt_embeds=one["npe"],
                     negative_pooled_prompt_embeds=one["npooled"], ip_adapter_image_embeds=[one["img"]], output_type="latent",
                     previewer_scheduler=LCMSingleStepScheduler.from_config(p.scheduler.config),
                     init_noise=torch.cat([one["init_noise"]] * 2), guidance_scale=7.0, **LOOP, **kw, **extra)
        return out.float().cpu(), row
    a, row = run(True)
    b, _ = run(True)
    c, _ = run(False)
    assert a.shape[0] == 2 and torch.isfinite(a).all() and len(row) > 0
    assert torch.equal(a, b) and not torch.equal(a, c)


def test_cli_pag_equals_python_api(tmp_path, dev):
    from PIL import Image
    import instantir_amd.infer as cli
    src, out = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    Image.fromarray(np.random.default_rng(0).integers(0, 255, (96, 96, 3), dtype=np.uint8)).save(src / "a.png")
    args = cli.build_parser().parse_args(["--test_path", str(src), "--out_path", str(out), "--synthetic", "tiny",
                                          "--num_inference_steps", "4", "--width", "128", "--height", "128", "--batch_size", "1",
                                          "--cfg", "5.0", "--pag_scale", "2.5", "--pag_adaptive_scale", "0.001",
                                          "--pag_layers", "mid,up_blocks.0"])
    orig = cli.resize_img
    cli.resize_img = lambda im, **kw: orig(im, max_side=128, min_side=128, **kw)
    try:
        torch.manual_seed(7)               # the synthetic VAE encode draws its eps from the global generator
        cli.main(args, dev)
        im, size = cli.resize_img(Image.open(src / "a.png").convert("RGB"), width=128, height=128)
    finally:
        cli.resize_img = orig
    got = np.asarray(Image.open(out / "a.png"))
    torch.manual_seed(7)
    pipe, lcm = cli.build_pipeline(args, dev)
    pipe.enable_pag(["mid", "up_blocks.0"])
    cfg = pipe.cfg
    g = torch.Generator().manual_seed(42)
    kw = dict(prompt_embeds=torch.randn(1, cfg.text_len, cfg.cross_attention_dim, generator=g),
              pooled_prompt_embeds=torch.randn(1, cfg.pooled_dim, generator=g),
              negative_prompt_embeds=torch.randn(1, cfg.text_len, cfg.cross_attention_dim, generator=g),
              negative_pooled_prompt_embeds=torch.randn(1, cfg.pooled_dim, generator=g),
              ip_adapter_image_embeds=[torch.randn(2, 1, cfg.resampler.seq_len, cfg.resampler.embedding_dim, generator=g)])
    rec = pipe(image=[im], num_inference_steps=4, generator=torch.Generator(device=dev).manual_seed(42), guidance_scale=5.0,
               previewer_scheduler=lcm, preview_start=0.0, control_guidance_end=1.0, pag_scale=2.5, pag_adaptive_scale=0.001,
               **kw).images[0]
    want = np.asarray(rec.resize([size[0], size[1]], Image.BILINEAR))
    assert got.shape == want.shape and np.array_equal(got, want)


def test_config1_geometry_one_step_with_pag(dev, pag_oracle_attn):
    """configs[1]'s geometry (1024^2, cfg 7, B = 1, 3 main-UNet rows) for one DDPM step at t = 501 with PAG on `mid`, against the
    PAG'd CPU oracle; two calls bit-identical.  Bar: 50 dB."""
    from instantir_amd import pag, weights as W
    from instantir_amd.config import UNetConfig
    from instantir_amd.pipeline import InstantIRPipeline
    from instantir_amd.schedulers import DDPMScheduler, LCMSingleStepScheduler
    from oracle import nets, sched
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
    pipe.enable_pag("mid")
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
    paths = pag.select("mid", pag.attn1_paths(cfg))
    with torch.no_grad():
        acp = sched.make_alphas_cumprod()
        t = 501
        x = sched.add_noise(acp, lq, noise, [t])
        xin = torch.cat([x] * 2)
        ctx, text = torch.cat([npe, pe]), torch.cat([npooled, pooled])
        tid = torch.tensor([[1024.0, 1024, 0, 0, 1024, 1024]]).repeat(2, 1)
        ip_main = nets.image_projection(P, [feats], cfg.resampler)[0]
        ip_prev = nets.image_projection(P, [feats], cfg.resampler, L)[0]
        preview = sched.lcm_step(acp, nets.unet_forward(P, cfg, xin, t, ctx, text, tid, ip_prev, lora=L), t, xin)
        down, mid = nets.aggregator_forward(PA, cfg, torch.cat([lq] * 2), t, preview, text, tid)
        e = lr.pag_unet(paths, B)(P, cfg, xin, t, ctx, text, tid, ip_main, down, mid)
        u, c, p = e.chunk(3)
        eps = u + 7.0 * (c - u) + 3.0 * (c - p)
        want, _ = sched.ddpm_step(acp, eps, t, x, 1, noise=sn[0], prev_t=-1)
    v = psnr(got, want)
    print(f"configs[1] geometry, one step with PAG (mid): latent PSNR vs CPU fp32 oracle {v:.1f} dB")
    assert v >= 50.0, v
