"""The tiny-geometry denoising loop shared by the GPU loop tests: the seeded environment, the pipeline under test, the fp32 CPU
oracle loops (oracle.pipeline.denoise; the sigma-scheduler loop here) and the guidance methods as those loops' two hooks --
`main_unet` (PAG / SEG: the main UNet returns [u;] c; p) and `guide` (the row groups' combination into eps).  oracle/nets.py is
not edited: the perturbed self-attentions are monkeypatch fixtures (`pag_oracle_attn` here, seg_ref.swap_attn_self)."""
import inspect
import math

import numpy as np
import pytest
import torch

import apg_ref
import seg_ref
import test_sigma_schedulers_cpu as spec

PHASES = dict(preview_start=0.25, control_guidance_end=0.75)     # creative tail, Aggregator-only head, previewed middle
LOOP = dict(num_inference_steps=8, **PHASES)


# ---- environment, pipeline, PSNR ------------------------------------------------------------------------------------------
def tiny_env(noises=8):
    from instantir_amd import weights as W
    from instantir_amd.config import UNetConfig
    cfg = UNetConfig.tiny()
    sd = W.synth_state_dict(W.unet_specs(cfg), 11)
    sda = W.synth_state_dict(W.aggregator_specs(cfg), 12)
    lora = W.synth_state_dict(W.lora_specs(cfg), 13)
    g = torch.Generator().manual_seed(42)
    B, H = 2, 16
    inp = dict(
        B=B, H=H,
        lq=torch.randn(B, 4, H, H, generator=g) * 0.8,
        pe=torch.randn(B, cfg.text_len, cfg.cross_attention_dim, generator=g).half().float(),
        pooled=torch.randn(B, cfg.pooled_dim, generator=g).half().float(),
        npe=torch.randn(B, cfg.text_len, cfg.cross_attention_dim, generator=g).half().float(),
        npooled=torch.randn(B, cfg.pooled_dim, generator=g).half().float(),
        img=torch.randn(2, B, cfg.resampler.seq_len, cfg.resampler.embedding_dim, generator=g).half().float(),
        init_noise=torch.randn(B, 4, H, H, generator=g),
        noises=[torch.randn(B, 4, H, H, generator=g) for _ in range(noises)],
    )
    return cfg, sd, sda, lora, inp


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from instantir_amd import lib
    lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def env(dev):
    return tiny_env()


def params(env):
    """P, PA, L: the state dicts as fp32, the LoRA with its scaling (lora_alpha = 16)"""
    cfg, sd, sda, lora, _ = env
    L = {k: v.float() for k, v in lora.items()}
    L["scaling"] = 16.0 / cfg.lora_rank
    return {k: v.float() for k, v in sd.items()}, {k: v.float() for k, v in sda.items()}, L


def pipe(env, sched=None):
    from instantir_amd.pipeline import InstantIRPipeline
    from instantir_amd.schedulers import DDIMScheduler
    cfg, sd, sda, lora, _ = env
    p = InstantIRPipeline(cfg, sd, scheduler=sched if sched is not None else DDIMScheduler())
    p.aggregator.load_state_dict(sda)
    p.prepare_previewers(lora, lora_alpha=16)
    return p


def call(pipe, inp, guidance_scale=7.0, **kw):
    """The final latents (fp32, CPU); without CFG the negative embeds stay out and the IP embeds are the cond group alone."""
    from instantir_amd.schedulers import LCMSingleStepScheduler
    lcm = LCMSingleStepScheduler.from_config(pipe.scheduler.config)
    cfg_on = guidance_scale > 1
    neg = dict(negative_prompt_embeds=inp["npe"], negative_pooled_prompt_embeds=inp["npooled"]) if cfg_on else {}
    return pipe(image=inp["lq"], prompt_embeds=inp["pe"], pooled_prompt_embeds=inp["pooled"],
                ip_adapter_image_embeds=[inp["img"] if cfg_on else inp["img"][-1:]], output_type="latent", previewer_scheduler=lcm,
                init_noise=inp["init_noise"], guidance_scale=guidance_scale, **neg, **kw).images.float().cpu()


def sigma_sched(kind, karras=False):
    from instantir_amd import schedulers as S
    if kind == "euler":
        return S.EulerDiscreteScheduler(use_karras_sigmas=karras)
    if kind == "euler_a":
        return S.EulerAncestralDiscreteScheduler()
    return S.DPMSolverMultistepScheduler(use_karras_sigmas=karras,
                                         algorithm_type="sde-dpmsolver++" if kind == "dpm_sde" else "dpmsolver++")


def psnr(got, want, name=None):
    """Peak (of `want`) signal-to-noise ratio in dB, in fp64; recorded by conftest.record_psnr under `name` when given."""
    from conftest import record_psnr
    mse = ((got.double() - want.double()) ** 2).mean().item()
    peak = want.abs().max().item()
    v = 10 * math.log10(peak * peak / max(mse, 1e-30))
    if name:
        record_psnr(name, v)
    return v


def psnr_by_caller(prefix):
    """psnr(got, want) that records every value as `<prefix>.<calling function>`"""
    return lambda got, want: psnr(got, want, prefix + "." + inspect.stack()[1].function)


# ---- the oracle loops -------------------------------------------------------------------------------------------------------
def denoise(env, guidance_scale=7.0, **kw):
    """oracle.pipeline.denoise on the environment's inputs (DDIM unless `sampler` says otherwise)"""
    from oracle import pipeline as OP
    cfg, inp = env[0], env[4]
    P, PA, L = params(env)
    do_cfg = guidance_scale > 1
    return OP.denoise(P, PA, L, cfg, inp["lq"], inp["pe"], inp["pooled"], inp["img"] if do_cfg else inp["img"][-1:],
                      negative_prompt_embeds=inp["npe"] if do_cfg else None, negative_pooled=inp["npooled"] if do_cfg else None,
                      init_noise=inp["init_noise"], guidance_scale=guidance_scale, **kw)


def ref_step(e, x, coef, m_prev, noise):
    """The step kernels' fp32 op order: x0 = (x - sb*e)/sa; prev = k0*x0 + kx*x (+ ke*e) (+ kh*m) (+ kn*noise)."""
    g, sb, sa, k0, kx, ke, kn, kh = [torch.tensor(c, dtype=torch.float32) for c in coef]
    x0 = (x - sb * e) / sa
    pv = k0 * x0 + kx * x
    if float(ke) != 0:
        pv = pv + ke * e
    if m_prev is not None and float(kh) != 0:
        pv = pv + kh * m_prev
    if noise is not None and float(kn) != 0:
        pv = pv + kn * noise
    return pv, x0


def ulps(a, b):
    """max |a - b| in fp32 ulps of max(|a|, |b|), floored at 2^-10 of the tensor's range (cancellation near zero)"""
    d = (a.double() - b.double()).abs()
    floor = max(b.abs().max().item() * 2.0 ** -10, 1e-30)
    u = torch.finfo(torch.float32).eps * torch.maximum(a.abs(), b.abs()).double().clamp_min(floor)
    return (d / u).max().item()


def sigma_denoise(env, kind, n, guidance_scale=5.0, preview_start=0.0, control_guidance_end=1.0, step_noises=None, karras=False,
                  adastep_restore=False, main_unet=None, guide=None):
    """fp32 CPU loop, pipelines/sdxl_instantir.py:1385-1660 with a sigma scheduler (CFG): add_noise in the scheduler's space,
    UNet / Aggregator input scale_model_input(cat([x]*2), t) at the float t, LCM preview on the scaled input at int(t),
    the step from the fp64 restatement (spec_*) applied in fp32.  `main_unet` / `guide`: as in oracle.pipeline.denoise, `t` the
    float timestep and `coef` the step's (sb, sa) as fp32."""
    from oracle import nets, sched
    cfg, inp = env[0], env[4]
    P, PA, L = params(env)
    B = inp["B"]
    acp = sched.make_alphas_cumprod()
    if kind.startswith("euler"):
        ts, sig = spec.spec_euler_table(n, "leading", karras)
    else:
        ts, sig = spec.spec_dpm_table(n, "leading", karras)
    keep, previewing = sched.gating_tables(n, 0.0, control_guidance_end, preview_start, 1.0)
    tid = torch.tensor([[128.0, 128, 0, 0, 128, 128]]).repeat(2 * B, 1)
    ctx, text = torch.cat([inp["npe"], inp["pe"]]), torch.cat([inp["npooled"], inp["pooled"]])
    image = torch.cat([inp["lq"]] * 2)
    ip_main = nets.image_projection(P, [inp["img"]], cfg.resampler)[0]
    ip_prev = nets.image_projection(P, [inp["img"]], cfg.resampler, L)[0]
    vp = kind.startswith("dpm")
    a0 = 1 / math.sqrt(sig[0] ** 2 + 1)
    x = (a0 * inp["lq"] + (sig[0] * a0) * inp["init_noise"]) if vp else inp["lq"] + sig[0] * inp["init_noise"]
    m = None
    preview_factor = torch.ones(B, 1, 1, 1)
    previewer_mean = torch.zeros_like(x)
    down = mid = None
    for i in range(n):
        t = ts[i]
        c_in = 1.0 if vp else float(np.float32(1 / math.sqrt(sig[i] ** 2 + 1)))
        xin = torch.cat([x] * 2) * c_in
        cond_scale = torch.cat([preview_factor.clamp(0.0, 1.0) * keep[i]] * 2)
        if (cond_scale > 0.1).sum().item() > 0:
            if previewing[i] > 0:
                eps1 = nets.unet_forward(P, cfg, xin, t, ctx, text, tid, ip_prev, lora=L)
                preview = sched.lcm_step(acp, eps1, int(t), xin)
            else:
                preview = image
            down, mid = nets.aggregator_forward(PA, cfg, image, t, preview, text, tid)
        down = [s * cond_scale for s in down]
        mid = mid * cond_scale
        if kind == "euler":
            coef = spec.spec_euler_coef(sig, i)
        elif kind == "euler_a":
            coef = spec.spec_euler_coef(sig, i, ancestral=True)
        else:
            coef = spec.spec_dpm_coef(sig, i, spec.spec_dpm_second_order(i, n), sde=kind == "dpm_sde")
        eps = (main_unet or nets.unet_forward)(P, cfg, xin, t, ctx, text, tid, ip_main, down, mid)
        rows = eps.chunk(eps.shape[0] // B)
        u, c = rows[:2]
        eps = u + guidance_scale * (c - u) if guide is None else guide(rows, i, t, x, (np.float32(coef[0]), np.float32(coef[1])))
        c32 = [0.0] + [float(np.float32(v)) for v in coef[:6]] + [float(np.float32(coef[6]))]
        nz = step_noises[i] if step_noises is not None else None
        x_next, x0 = ref_step(eps, x, c32, m, nz)
        m = x0
        if adastep_restore:
            pv = preview[B:].float()
            pred_x0_l2 = (pv - x0).pow(2).sum(dim=(1, 2, 3))
            previewer_l2 = (pv - previewer_mean).pow(2).sum(dim=(1, 2, 3))
            previewer_mean = preview[B:]
            preview_factor = (pred_x0_l2 / previewer_l2).reshape(-1, 1, 1, 1)
        x = x_next
    return x


# ---- `main_unet` hooks: the perturbed row group ---------------------------------------------------------------------------
_PAG = {"paths": None, "ident_from": 0}


@pytest.fixture
def pag_oracle_attn(monkeypatch):
    """oracle.nets.attn_self with the identity map on rows [ident_from, R) of the selected layers while _PAG['paths'] is set."""
    from oracle import nets
    orig = nets.attn_self

    def attn_self(P, path, x, heads, lora=None):
        out = orig(P, path, x, heads, lora)
        if _PAG["paths"] is not None and path in _PAG["paths"]:
            k = _PAG["ident_from"]
            out = torch.cat([out[:k], nets.linear(P, path + ".to_out.0", nets.linear(P, path + ".to_v", x[k:], lora), lora)])
        return out
    monkeypatch.setattr(nets, "attn_self", attn_self)
    yield
    _PAG["paths"] = None


def pag_unet(paths, B):
    """The main UNet on [xin rows; copies of the last B (cond) rows] with the perturbed rows' self-attention the identity
    (needs `pag_oracle_attn`)."""
    def unet(P, cfg, xin, t, ctx, text, tid, ip, down, mid):
        from oracle import nets
        R = xin.shape[0]
        c = slice(R - B, R)
        ext = lambda v: torch.cat([v, v[c]])
        _PAG["paths"], _PAG["ident_from"] = set(paths), R
        try:
            return nets.unet_forward(P, cfg, ext(xin), t, ext(ctx), ext(text), ext(tid), ext(ip), [ext(d) for d in down], ext(mid))
        finally:
            _PAG["paths"] = None
    return unet


def seg_unet(paths, B, sigma):
    """The same row groups, the copies' selected self-attentions in SEG form (needs seg_ref.swap_attn_self)."""
    return lambda *args: seg_ref.seg_unet(*args, paths, B, sigma)


# ---- `guide` hooks: rows = ([u,] c[, p]) -> eps -----------------------------------------------------------------------------
def cfg_guide(g):
    return lambda rows, i, t, x, coef: rows[0] + g * (rows[1] - rows[0]) if len(rows) > 1 else rows[0]


def perturbed(g, scale, adaptive=0.0, base=None):
    """(u + g (c - u)) + s_t (c - p), or c + s_t (c - p) without CFG (g <= 1); s_t = max(scale - adaptive (1000 - t), 0).
    `base`: another hook for the CFG part (`apg`)."""
    base = base or cfg_guide(g)

    def guide(rows, i, t, x, coef):
        c, p = rows[-2], rows[-1]
        s_t = max(scale - adaptive * (1000 - float(t)), 0.0)
        return base(rows[:-1], i, t, x, coef) + s_t * (c - p)
    return guide


def apg(g, par):
    """The fp32 guided eps of apg_ref.apg_eps, par = (eta, norm_threshold, momentum); the running average lives here and
    starts afresh at step 0 (where the momentum is 0, as in the pipeline)."""
    state = {}

    def guide(rows, i, t, x, coef):
        first = i == 0
        eps, A, _, _ = apg_ref.apg_eps(rows[0], rows[1], x, None if first else state["A"], [g, float(coef[0]), float(coef[1])],
                                       par[0], par[1], 0.0 if first else par[2], fp32=True)
        state["A"] = A.float()
        return eps.float()
    return guide


_ORACLES = {}


def guided(env, kind, layers=None, *, guidance_scale, scale=0.0, sigma=100.0, guidance_rescale=0.0, apg_par=None,
           num_inference_steps=8):
    """The DDIM oracle with eps = u + g (c - u) + s (c - p) (c + s (c - p) without CFG; with `apg_par` the CFG part is
    apg_ref's, as the step kernel composes them); `kind` None (no perturbed rows), "pag" or "seg".  Results are kept: the plain
    and PAG'd oracles serve several cases."""
    from instantir_amd import pag
    key = (kind, str(layers), guidance_scale, scale if kind else 0.0, sigma if kind == "seg" else 0.0, guidance_rescale, apg_par,
           num_inference_steps)
    if key not in _ORACLES:
        B = env[4]["B"]
        paths = pag.select(layers, pag.attn1_paths(env[0])) if kind else None
        unet = {None: None, "pag": pag_unet(paths, B), "seg": seg_unet(paths, B, sigma)}[kind]
        guide = apg(guidance_scale, apg_par) if apg_par is not None and guidance_scale > 1 else None
        if kind:
            guide = perturbed(guidance_scale, scale, base=guide)
        _ORACLES[key] = denoise(env, guidance_scale, main_unet=unet, guide=guide, guidance_rescale=guidance_rescale,
                                num_inference_steps=num_inference_steps, **PHASES)
    return _ORACLES[key]
