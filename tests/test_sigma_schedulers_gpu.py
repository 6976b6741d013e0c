"""GPU: the Euler / Euler-ancestral / DPM++ 2M schedulers on the HIP path -- iir_sched_step_hist(_f32) and
iir_pack_latent_dscale against fp32 torch, the public `.step()` over whole timetables, and the denoising loop at the tiny
geometry against the DDIM loop (Euler is DDIM in VP space) and against an fp32 CPU loop composed here from `oracle.nets`
with the fp64 scheduler restatement of tests/test_sigma_schedulers_cpu.py (tests/loop_ref.py: sigma_denoise)."""
import math
import os

import numpy as np
import pytest
import torch

import loop_ref as lr
import test_sigma_schedulers_cpu as spec
from loop_ref import dev, env  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

BAR = 50.0


psnr = lr.psnr_by_caller("sigma")


# ---- kernels --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W", [(1, 128, 128), (2, 5, 7), (2, 16, 16)])
@pytest.mark.parametrize("cfg", [False, True])
@pytest.mark.parametrize("extra", ["plain", "noise", "rescale"])
def test_sched_step_hist_matches_fp32(dev, B, H, W, cfg, extra):
    from instantir_amd import ops
    if extra == "rescale" and not cfg:
        extra = "noise"
    g = torch.Generator().manual_seed(B * 1000 + H * W)
    C, lde, R = 4, 8, B * (2 if cfg else 1)
    HW = H * W
    eps16 = (torch.randn(R * HW, lde, generator=g)).half()
    x = torch.randn(B, C, H, W, generator=g) * 3
    m = torch.randn(B, C, H, W, generator=g)
    nz = torch.randn(B, C, H, W, generator=g) if extra == "noise" else None
    fac = torch.tensor([0.8, 1.3][:B]) if extra == "rescale" else None
    coef = [6.5, 0.93, 0.37, 0.41, 0.98, 0.12, 0.07 if nz is not None else 0.0, -0.031]
    hist = m.clone().to(dev)
    prev, x0 = torch.empty(B, C, H, W, device=dev), torch.empty(B, C, H, W, device=dev)
    ops.sched_step_hist(eps16.to(dev), B, torch.tensor(coef).to(dev), x.to(dev), hist, prev, noise=None if nz is None else nz.to(dev),
                        cfg=cfg, x0_out=x0, eps_factor=None if fac is None else fac.to(dev))
    torch.cuda.synchronize()
    e = eps16.float()[:, :C].reshape(R, H, W, C).permute(0, 3, 1, 2)
    if cfg:
        u, t = e[:B], e[B:]
        e = u + torch.tensor(coef[0]) * (t - u)
        if fac is not None:
            e = e * fac.view(B, 1, 1, 1)
    want, want_x0 = lr.ref_step(e, x, coef, m, nz)
    assert lr.ulps(prev.cpu(), want) <= 4 and lr.ulps(x0.cpu(), want_x0) <= 4
    assert torch.equal(hist.cpu(), x0.cpu())                 # the plane now holds this step's x0


def test_sched_step_hist_never_reads_history_when_kh_is_zero(dev):
    from instantir_amd import ops
    g = torch.Generator().manual_seed(5)
    B, C, H, W = 2, 4, 9, 11
    eps16 = torch.randn(2 * B * H * W, 4, generator=g).half().to(dev)
    x = torch.randn(B, C, H, W, generator=g).to(dev)
    coef = torch.tensor([5.0, 0.9, 0.4, 0.5, 0.9, 0.0, 0.0, 0.0]).to(dev)
    hist = torch.full((B, C, H, W), float("nan"), device=dev)
    prev, x0 = torch.empty_like(x), torch.empty_like(x)
    ops.sched_step_hist(eps16, B, coef, x, hist, prev, cfg=True, x0_out=x0)
    ref = torch.empty_like(x)
    ops.sched_step(eps16, B, coef, x, ref, cfg=True)          # k_h == 0: the existing step, bit for bit
    hf = torch.full((B * C * H * W,), float("nan"), device=dev)
    e32, x32 = torch.randn(B * C * H * W, generator=g).to(dev), x.flatten().clone()
    p32 = torch.empty_like(x32)
    ops.sched_step_hist_f32(e32, x32, coef, hf, p32)
    torch.cuda.synchronize()
    assert torch.isfinite(prev).all() and torch.isfinite(p32).all()
    assert torch.equal(prev, ref) and torch.equal(hist, x0) and torch.isfinite(hf).all()


def test_update_bits_match_the_recorded_library(dev, golden_dir):
    """Every output buffer of the exported pack / CFG-rescale / scheduler-step entries, replayed on seeded inputs, against the
    bits recorded in tests/golden/sched_update_bits.npz (tests/golden/make_sched_update_bits.py) before the kernels behind
    those entries were folded into one per family."""
    from golden.make_sched_update_bits import replay
    want = np.load(os.path.join(golden_dir, "sched_update_bits.npz"))
    got = replay()
    assert sorted(got) == sorted(want.files)
    bad = [k for k in want.files if not np.array_equal(got[k], want[k])]
    assert not bad, bad


def test_keep_and_apg_update_bits_match_the_recorded_library(dev, golden_dir):
    """The restore-map and APG forms of the step (keep x hist x pag x cfg, apg x keep x hist) through ops.sched_step /
    ops.apg_project, against the bits recorded in tests/golden/sched_update_bits_keep_apg.npz before the positional step entries
    were replaced by iir_sched_step on a descriptor: a pointer in the wrong field of the descriptor shows here."""
    from golden.make_sched_update_bits import replay_keep_apg
    want = np.load(os.path.join(golden_dir, "sched_update_bits_keep_apg.npz"))
    got = replay_keep_apg()
    assert sorted(got) == sorted(want.files)
    bad = [k for k in want.files if not np.array_equal(got[k], want[k])]
    assert not bad, bad


@pytest.mark.parametrize("B,H,W,rep", [(1, 128, 128, 2), (2, 5, 7, 1), (2, 16, 16, 2)])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_device_scale_pack_bit_identical_to_host_scale(dev, B, H, W, rep, dtype):
    from instantir_amd import ops
    x = (torch.randn(B, 4, H, W, generator=torch.Generator().manual_seed(H)) * 9).to(dev)
    for s in (1.0, 0.0862, 0.7071067690849304):
        s32 = float(np.float32(s))
        a = torch.full((rep * B * H * W, 8), 7.0, dtype=dtype, device=dev)
        b = a.clone()
        ops.pack_latent(x, a, rep=rep, scale=s32)
        ops.pack_latent_dscale(x, b, torch.tensor([s32], device=dev), rep=rep)
        torch.cuda.synchronize()
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))


# ---- public .step() -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["euler", "euler_karras", "euler_a", "dpm", "dpm_karras", "dpm_sde", "dpm_order1"])
def test_public_step_over_a_timetable(dev, name):
    from instantir_amd import schedulers as S
    mk = {"euler": lambda: S.EulerDiscreteScheduler(), "euler_karras": lambda: S.EulerDiscreteScheduler(use_karras_sigmas=True),
          "euler_a": lambda: S.EulerAncestralDiscreteScheduler(),
          "dpm": lambda: S.DPMSolverMultistepScheduler(timestep_spacing="trailing"),
          "dpm_karras": lambda: S.DPMSolverMultistepScheduler(use_karras_sigmas=True),
          "dpm_sde": lambda: S.DPMSolverMultistepScheduler(algorithm_type="sde-dpmsolver++"),
          "dpm_order1": lambda: S.DPMSolverMultistepScheduler(solver_order=1)}[name]
    sch = mk()
    n = 12
    sch.set_timesteps(n)
    euler = name.startswith("euler")
    if euler:
        _, sig = spec.spec_euler_table(n, sch.config.timestep_spacing, sch.use_karras_sigmas)
    else:
        _, sig = spec.spec_dpm_table(n, sch.config.timestep_spacing, sch.use_karras_sigmas)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 4, 8, 8, generator=g) * sch.init_noise_sigma
    xg, xr, m = x.to(dev), x.double(), None
    for i, t in enumerate(sch.timesteps):
        e = torch.randn(2, 4, 8, 8, generator=g)
        nz = torch.randn(2, 4, 8, 8, generator=g)
        out = sch.step(e.to(dev), t, xg, variance_noise=nz.to(dev))
        if euler:
            c = spec.spec_euler_coef(sig, i, ancestral=name == "euler_a")
        else:
            c = spec.spec_dpm_coef(sig, i, spec.spec_dpm_second_order(i, n, sch.config.solver_order),
                                   sde=name == "dpm_sde")
        sb, sa, k0, kx, ke, kn, kh = c
        x0 = (xr - sb * e.double()) / sa
        xr = k0 * x0 + kx * xr + ke * e.double() + kn * nz.double() + (kh * m if kh != 0 else 0)
        m = x0
        assert torch.allclose(out.pred_original_sample.cpu().double(), x0, rtol=1e-4, atol=1e-4 * x0.abs().max().item())
        xg = out.prev_sample
        assert torch.allclose(xg.cpu().double(), xr, rtol=1e-4, atol=1e-4 * xr.abs().max().item()), (i, (xg.cpu().double() - xr).abs().max())
    assert sch.step_index == n
    sch.set_timesteps(n)
    assert sch.step_index is None


# ---- the denoising loop -------------------------------------------------------------------------------------------------------
PHASES = lr.PHASES


@pytest.mark.parametrize("kind,karras,noises", [("dpm", True, False), ("dpm_sde", False, True), ("euler", True, False),
                                               ("euler_a", False, True)])
def test_loop_matches_fp32_oracle(env, kind, karras, noises):
    inp = env[4]
    n = 8
    kw = dict(num_inference_steps=n, guidance_scale=5.0, **PHASES)
    sn = inp["noises"] if noises else None
    want = lr.sigma_denoise(env, kind, n, step_noises=sn, karras=karras, **PHASES)
    got = lr.call(lr.pipe(env, lr.sigma_sched(kind, karras)), inp, step_noises=sn, **kw)
    p = psnr(got, want)
    print(f"{kind} karras={karras}: latent PSNR vs fp32 oracle {p:.1f} dB")
    assert torch.isfinite(got).all() and p >= BAR, p


def test_adastep_restore_dpm_matches_oracle(env):
    inp = env[4]
    want = lr.sigma_denoise(env, "dpm", 6, karras=True, adastep_restore=True)
    got = lr.call(lr.pipe(env, lr.sigma_sched("dpm", True)), inp, num_inference_steps=6, guidance_scale=5.0, adastep_restore=True)
    p = psnr(got, want)
    assert torch.isfinite(got).all() and p >= BAR, p


def test_euler_is_the_ddim_loop_in_vp_space(env):
    """Per step through callback_on_step_end: x_VE / sqrt(sigma_{i+1}^2 + 1) against the DDIM loop's x_VP, steps 0..n-2."""
    from instantir_amd.schedulers import DDIMScheduler
    inp = env[4]
    n = 6
    seen = {"e": [], "d": []}

    def rec(key):
        def cb(pipe, i, t, kw):
            seen[key].append(kw["latents"].float().cpu().clone())
            return {}
        return cb
    e = lr.sigma_sched("euler")
    lr.call(lr.pipe(env, e), inp, num_inference_steps=n, guidance_scale=5.0, callback_on_step_end=rec("e"), **PHASES)
    lr.call(lr.pipe(env, DDIMScheduler()), inp, num_inference_steps=n, guidance_scale=5.0, callback_on_step_end=rec("d"), **PHASES)
    for i in range(n - 1):
        s = float(e.sigmas[i + 1])
        p = psnr(seen["e"][i] / math.sqrt(s * s + 1), seen["d"][i])
        assert p >= 60.0, (i, p)


def test_graphs_on_off_and_repeat_calls_bit_identical(env):
    from instantir_amd.schedulers import DDPMScheduler
    inp = env[4]
    kw = dict(num_inference_steps=6, guidance_scale=5.0, step_noises=inp["noises"], **PHASES)
    pipe = lr.pipe(env, lr.sigma_sched("dpm_sde", False))
    pipe.use_graphs = False
    eager = lr.call(pipe, inp, **kw)
    pipe.use_graphs = True
    g1 = lr.call(pipe, inp, **kw)
    g2 = lr.call(pipe, inp, **kw)                   # the loop is adopted: the history is reset
    assert torch.equal(eager, g1) and torch.equal(g1, g2)
    dd = DDPMScheduler()
    pipe_d = lr.pipe(env, dd)
    want_d = lr.call(pipe_d, inp, **kw)
    dpm = pipe.scheduler
    pipe.scheduler = dd
    assert torch.equal(lr.call(pipe, inp, **kw), want_d)
    pipe.scheduler = dpm
    assert torch.equal(lr.call(pipe, inp, **kw), g1)


def test_prompt_embeds_replaced_mid_loop_keeps_history(env):
    """A callback that replaces prompt_embeds rebuilds the loop; the DPM++ history is carried over, so returning the same
    values (a new tensor) gives the uninterrupted result bit for bit."""
    inp = env[4]
    kw = dict(num_inference_steps=6, guidance_scale=5.0, **PHASES)
    pipe = lr.pipe(env, lr.sigma_sched("dpm", True))
    want = lr.call(pipe, inp, **kw)

    def cb(p, i, t, d):
        return {"prompt_embeds": d["prompt_embeds"].clone()} if i == 2 else {}
    got = lr.call(pipe, inp, callback_on_step_end=cb, callback_on_step_end_tensor_inputs=["latents", "prompt_embeds"], **kw)
    assert torch.equal(got, want)


def test_timesteps_argument_refused(env):
    inp = env[4]
    with pytest.raises(ValueError, match="timesteps"):
        lr.call(lr.pipe(env, lr.sigma_sched("euler")), inp, timesteps=[999, 500, 1], guidance_scale=5.0)


def test_cli_dpmpp_2m_karras_equals_python_api(tmp_path, dev):
    from PIL import Image
    import instantir_amd.infer as cli
    from instantir_amd.schedulers import DPMSolverMultistepScheduler
    src, out = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    Image.fromarray(np.random.default_rng(0).integers(0, 255, (96, 96, 3), dtype=np.uint8)).save(src / "a.png")
    args = cli.build_parser().parse_args(["--test_path", str(src), "--out_path", str(out), "--synthetic", "tiny",
                                          "--num_inference_steps", "4", "--width", "128", "--height", "128", "--batch_size", "1",
                                          "--cfg", "5.0", "--scheduler", "dpmpp_2m", "--karras"])
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
    pipe.scheduler = DPMSolverMultistepScheduler.from_config(pipe.scheduler.config, use_karras_sigmas=True)
    cfg = pipe.cfg
    g = torch.Generator().manual_seed(42)
    kw = dict(prompt_embeds=torch.randn(1, cfg.text_len, cfg.cross_attention_dim, generator=g),
              pooled_prompt_embeds=torch.randn(1, cfg.pooled_dim, generator=g),
              negative_prompt_embeds=torch.randn(1, cfg.text_len, cfg.cross_attention_dim, generator=g),
              negative_pooled_prompt_embeds=torch.randn(1, cfg.pooled_dim, generator=g),
              ip_adapter_image_embeds=[torch.randn(2, 1, cfg.resampler.seq_len, cfg.resampler.embedding_dim, generator=g)])
    rec = pipe(image=[im], num_inference_steps=4, generator=torch.Generator(device=dev).manual_seed(42), guidance_scale=5.0,
               previewer_scheduler=lcm, preview_start=0.0, control_guidance_end=1.0, **kw).images[0]
    want = np.asarray(rec.resize([size[0], size[1]], Image.BILINEAR))
    assert got.shape == want.shape and np.array_equal(got, want)
    assert os.path.isfile(out / "a.png")
