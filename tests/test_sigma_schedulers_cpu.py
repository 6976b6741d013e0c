"""CPU: the Euler, Euler-ancestral and DPM++ 2M schedulers' host side against an fp64 restatement of diffusers 0.28.1
(timetables, sigmas, init_noise_sigma, scale_model_input, step coefficients), the spec's anchors, from_config /
from_pretrained across classes, the refused options, ABI argument checks of the new HIP entries and the CLI flags.

`spec_*` below is written from the formulas alone (no code shared with instantir_amd.schedulers) and is reused by
tests/test_sigma_schedulers_gpu.py as the oracle's scheduler."""
import ctypes
import json
import math

import numpy as np
import pytest
import torch

from instantir_amd import schedulers as S

T = 1000


def spec_sigma_train():
    """sigma(t) over t = 0..999 from the project's fp32 abar table (scaled_linear 0.00085..0.012)."""
    betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, T, dtype=torch.float32) ** 2
    acp = torch.cumprod(1.0 - betas, dim=0)
    return (((1 - acp) / acp) ** 0.5).numpy().astype(np.float32)


def spec_sigma_to_t(sig, log_tab):
    ls = math.log(max(sig, 1e-10))
    lo = 0
    for k in range(len(log_tab)):            # last training index whose log-sigma is <= log(sig)
        if ls - float(log_tab[k]) >= 0:
            lo = k
    lo = min(lo, len(log_tab) - 2)
    w = (float(log_tab[lo]) - ls) / (float(log_tab[lo]) - float(log_tab[lo + 1]))
    w = min(max(w, 0.0), 1.0)
    return (1 - w) * lo + w * (lo + 1)


def spec_karras(smax, smin, n):
    return [(smax ** (1 / 7) + (i / (n - 1) if n > 1 else 0.0) * (smin ** (1 / 7) - smax ** (1 / 7))) ** 7 for i in range(n)]


def spec_euler_table(n, spacing="leading", karras=False, offset=1):
    st = spec_sigma_train()
    if spacing == "leading":
        ts = [float(k * (T // n) + offset) for k in range(n)][::-1]
    elif spacing == "trailing":
        ts = [float(round(T - k * T / n) - 1) for k in range(n)]
    else:
        ts = [float(v) for v in np.linspace(0, 999, n, dtype=np.float32)][::-1]
    ts = [float(np.float32(t)) for t in ts]
    sig = [float(np.interp(t, np.arange(T), st)) for t in ts]
    if karras:
        sig = spec_karras(sig[0], sig[-1], n)
        ts = [float(np.float32(spec_sigma_to_t(s, np.log(st)))) for s in sig]
    return ts, [float(np.float32(s)) for s in sig] + [0.0]


def spec_dpm_table(n, spacing="leading", karras=False, offset=1):
    st = spec_sigma_train()
    if karras:
        sig = spec_karras(float(st[-1]), float(st[0]), n)
        ts = [int(round(spec_sigma_to_t(s, np.log(st)))) for s in sig]
    else:
        if spacing == "leading":
            ts = [k * (T // (n + 1)) + offset for k in range(n + 1)][::-1][:-1]
        elif spacing == "trailing":
            ts = [int(round(T - k * T / n)) - 1 for k in range(n)]
        else:
            ts = [int(v) for v in np.linspace(0, 999, n + 1).round()][::-1][:-1]
        sig = [float(np.interp(t, np.arange(T), st)) for t in ts]
    return ts, [float(np.float32(s)) for s in sig] + [0.0]


def spec_euler_coef(sig, i, ancestral=False):
    """(sb, sa, k_x0, k_x, k_eps, k_noise, k_h) in fp64."""
    s, sn = sig[i], sig[i + 1]
    if not ancestral:
        return (s, 1.0, 0.0, 1.0, sn - s, 0.0, 0.0)
    up = math.sqrt(sn ** 2 * (s ** 2 - sn ** 2) / s ** 2)
    down = math.sqrt(sn ** 2 - up ** 2)
    return (s, 1.0, 0.0, 1.0, down - s, up, 0.0)


def spec_dpm_coef(sig, i, second_order, sde=False):
    s, sn = sig[i], sig[i + 1]
    a, an = 1 / math.sqrt(s * s + 1), 1 / math.sqrt(sn * sn + 1)
    if sn == 0.0:
        return (s * a, a, 1.0, 0.0, 0.0, 0.0, 0.0)
    h = math.log(s / sn)
    emh = math.exp(-h)
    if sde:
        kx, base, kn = (sn * an) / (s * a) * emh, an * (1 - emh ** 2), sn * an * math.sqrt(1 - emh ** 2)
    else:
        kx, base, kn = (sn * an) / (s * a), -an * (emh - 1), 0.0
    if not second_order:
        return (s * a, a, base, kx, 0.0, kn, 0.0)
    r = math.log(sig[i - 1] / s) / h
    return (s * a, a, base * (1 + 1 / (2 * r)), kx, 0.0, kn, -base / (2 * r))


def spec_dpm_second_order(i, n, solver_order=2):
    """First step first order; the last step first order (final sigma 0)."""
    return solver_order == 2 and 0 < i < n - 1


def _close(a, b, rel=2e-6):
    return abs(a - b) <= rel * max(abs(a), abs(b), 1e-6)


# ---- anchors ---------------------------------------------------------------------------------------------------------
def test_spec_anchors():
    st = spec_sigma_train()
    assert round(float(st[999]), 4) == 14.6146 and round(float(st[0]), 4) == 0.0292
    e = S.EulerDiscreteScheduler()
    e.set_timesteps(30)
    assert round(float(e.sigmas[0]), 4) == 11.4769 and abs(e.init_noise_sigma - 11.5203) < 2e-4
    ek = S.EulerDiscreteScheduler(use_karras_sigmas=True)
    ek.set_timesteps(20)
    assert round(float(ek.sigmas[0]), 4) == 11.0283 and round(float(ek.sigmas[-2]), 5) == 0.04131
    assert abs(float(ek.timesteps[0]) - 951.0) < 0.05 and float(ek.timesteps[5]) != int(ek.timesteps[5])
    d = S.DPMSolverMultistepScheduler()
    d.set_timesteps(20)
    assert d.timesteps.tolist()[:2] == [941, 894] and d.timesteps.tolist()[-2:] == [95, 48]
    dk = S.DPMSolverMultistepScheduler(use_karras_sigmas=True)
    dk.set_timesteps(20)
    assert dk.timesteps.tolist() == [999, 962, 921, 876, 827, 772, 710, 640, 561, 474, 380, 285, 197, 123, 69, 35, 15, 6, 2, 0]


# ---- timetables, sigmas, init_noise_sigma, scale_model_input -----------------------------------------------------------
EULER_CASES = [(c, sp, k, n) for c in ("euler", "euler_a") for sp in ("leading", "trailing", "linspace") for k in (False, True)
               for n in (1, 4, 20, 30, 50) if not (k and (c == "euler_a" or n == 1))]      # Karras: Euler only, N >= 2


@pytest.mark.parametrize("cls,spacing,karras,n", EULER_CASES)
def test_euler_tables(cls, spacing, karras, n):
    C = S.EulerDiscreteScheduler if cls == "euler" else S.EulerAncestralDiscreteScheduler
    sch = C(timestep_spacing=spacing, use_karras_sigmas=karras)
    sch.set_timesteps(n)
    ts, sig = spec_euler_table(n, spacing, karras)
    assert sch.timesteps.dtype == torch.float32 and sch.sigmas.dtype == torch.float32
    assert len(sch.timesteps) == n and len(sch.sigmas) == n + 1
    for a, b in zip(sch.timesteps.tolist(), ts):
        assert abs(a - b) <= 1e-4 * max(1.0, abs(b)), (a, b)
    for a, b in zip(sch.sigmas.tolist(), sig):
        assert _close(a, b), (a, b)
    smax = max(sig)
    want = smax if spacing in ("trailing", "linspace") else math.sqrt(smax ** 2 + 1)
    assert _close(float(sch.init_noise_sigma), want)
    x = torch.randn(2, 4, 3, 3, dtype=torch.float64)
    for i, t in enumerate(sch.timesteps):
        got = sch.scale_model_input(x, t)
        assert torch.allclose(got, x / math.sqrt(sig[i] ** 2 + 1), rtol=1e-6)
        lc = sch.loop_coefficients(i)
        assert lc["t"] == float(sch.timesteps[i]) and lc["t_lcm"] == int(sch.timesteps[i])
        assert _close(lc["c_in"], 1 / math.sqrt(sig[i] ** 2 + 1))
        want_c = spec_euler_coef(sig, i, ancestral=cls == "euler_a")
        for a, b in zip(lc["coef"][1:], want_c):
            assert a == float(np.float32(a)) and abs(a - b) <= 1e-6 * max(1.0, abs(b)), (i, lc["coef"], want_c)
    noisy = sch.add_noise(x, torch.ones_like(x), sch.timesteps[:1].repeat(2))
    assert torch.allclose(noisy, x + sig[0], rtol=1e-6)


DPM_CASES = [(sp, k, n, a) for sp in ("leading", "trailing", "linspace") for k in (False, True) for n in (1, 2, 10, 20, 30)
             for a in ("dpmsolver++", "sde-dpmsolver++") if not (k and n == 1)]          # Karras: N >= 2


@pytest.mark.parametrize("spacing,karras,n,algo", DPM_CASES)
def test_dpm_tables_and_coefficients(spacing, karras, n, algo):
    sch = S.DPMSolverMultistepScheduler(timestep_spacing=spacing, use_karras_sigmas=karras, algorithm_type=algo)
    sch.set_timesteps(n)
    ts, sig = spec_dpm_table(n, spacing, karras)
    assert sch.timesteps.tolist() == ts and sch.timesteps.dtype == torch.int64
    for a, b in zip(sch.sigmas.tolist(), sig):
        assert _close(a, b), (a, b)
    assert sch.init_noise_sigma == 1.0 and sch.order == 2
    x = torch.randn(2, 4, 3, 3)
    assert sch.scale_model_input(x, sch.timesteps[0]) is x
    noisy = sch.add_noise(x, torch.ones_like(x), sch.timesteps[:1].repeat(2))
    a0 = 1 / math.sqrt(sig[0] ** 2 + 1)
    assert torch.allclose(noisy, a0 * x + sig[0] * a0, rtol=1e-5, atol=1e-6)
    for i in range(n):
        lc = sch.loop_coefficients(i)
        assert lc["c_in"] == 1.0 and lc["t"] == float(ts[i]) and lc["t_lcm"] == ts[i]
        want = spec_dpm_coef(sig, i, spec_dpm_second_order(i, n), sde=algo == "sde-dpmsolver++")
        for a, b in zip(lc["coef"][1:], want):
            assert abs(a - b) <= 2e-6 * max(1.0, abs(b)), (i, lc["coef"], want)
    assert lc["coef"][1:] == [sch.loop_coefficients(n - 1)["coef"][1], sch.loop_coefficients(n - 1)["coef"][2], 1.0, 0.0, 0.0, 0.0, 0.0]


def test_dpm_karras_repeated_timesteps_refused():
    sch = S.DPMSolverMultistepScheduler(use_karras_sigmas=True)
    with pytest.raises(ValueError, match="repeated"):
        sch.set_timesteps(200)


# ---- identities in exact arithmetic ----------------------------------------------------------------------------------
def _affine(sb, sa, k0, kx, ke, kn, kh):
    """(x, eps, m_prev) -> x' coefficients of the linear form."""
    return (k0 / sa + kx, -k0 * sb / sa + ke, kh)


def _ddim64(acp, t, t_prev, final=None):
    a_t = float(acp[t])
    a_p = float(acp[t_prev]) if t_prev >= 0 else final
    x0x, x0e = 1 / math.sqrt(a_t), -math.sqrt(1 - a_t) / math.sqrt(a_t)
    return (math.sqrt(a_p) * x0x, math.sqrt(a_p) * x0e + math.sqrt(1 - a_p))


@pytest.mark.parametrize("n", [4, 20, 30])
def test_euler_in_vp_space_is_ddim_eta0(n):
    """x_VP = x_VE / sqrt(sigma^2+1): an Euler step maps onto DDIM (eta = 0) on every step but the last."""
    betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, T, dtype=torch.float32) ** 2
    acp = torch.cumprod(1.0 - betas, dim=0).double()
    e = S.EulerDiscreteScheduler()
    e.set_timesteps(n)
    sig = [float(s) for s in e.sigmas]
    dd = S.DDIMScheduler()
    dd.set_timesteps(n)
    assert [int(t) for t in e.timesteps] == dd.timesteps.tolist()
    for i in range(n - 1):
        t, tp = int(e.timesteps[i]), int(e.timesteps[i + 1])
        s, sn = sig[i], sig[i + 1]
        a, an = 1 / math.sqrt(s * s + 1), 1 / math.sqrt(sn * sn + 1)
        # sigmas come from the fp32 table: redo DDIM from the same fp32 sigmas, abar = 1 / (sigma^2 + 1)
        acp_i = {t: 1 / (s * s + 1), tp: 1 / (sn * sn + 1)}
        kx, ke, _ = _affine(*spec_euler_coef(sig, i))
        got = (an * kx / a, an * ke)                    # x'_VP = an * x'_VE,  x_VE = x_VP / a
        want = _ddim64(acp_i, t, tp)
        assert all(abs(g - w) <= 1e-12 * max(1.0, abs(w)) for g, w in zip(got, want)), (i, got, want)
        assert abs(acp_i[t] - float(acp[t])) < 1e-6      # ... and those are the DDIM table's abar to fp32 rounding


@pytest.mark.parametrize("spacing", ["leading", "linspace", "trailing"])
@pytest.mark.parametrize("n", [3, 20])
def test_dpm_first_order_is_ddim_on_its_own_timesteps(spacing, n):
    sch = S.DPMSolverMultistepScheduler(solver_order=1, timestep_spacing=spacing)
    sch.set_timesteps(n)
    sig = [float(s) for s in sch.sigmas]
    for i in range(n):
        acp_i = {0: 1 / (sig[i] ** 2 + 1), 1: 1 / (sig[i + 1] ** 2 + 1)}
        got = _affine(*spec_dpm_coef(sig, i, False))[:2]
        want = _ddim64(acp_i, 0, 1 if i < n - 1 else -1, final=1.0)
        assert all(abs(g - w) <= 1e-12 * max(1.0, abs(w)) for g, w in zip(got, want)), (i, got, want)
        assert sch.loop_coefficients(i)["coef"][7] == 0.0


# ---- configuration ----------------------------------------------------------------------------------------------------
SDXL_CONFIG = {"_class_name": "EulerDiscreteScheduler", "_diffusers_version": "0.19.0.dev0", "beta_end": 0.012,
               "beta_schedule": "scaled_linear", "beta_start": 0.00085, "clip_sample": False, "interpolation_type": "linear",
               "num_train_timesteps": 1000, "prediction_type": "epsilon", "sample_max_value": 1.0, "set_alpha_to_one": False,
               "skip_prk_steps": True, "steps_offset": 1, "timestep_spacing": "leading", "trained_betas": None,
               "use_karras_sigmas": False}


@pytest.mark.parametrize("src", ["ddpm", "ddim", "lcm", "euler", "euler_a", "dpm"])
def test_from_config_across_classes(src):
    mk = {"ddpm": S.DDPMScheduler, "ddim": S.DDIMScheduler, "lcm": S.LCMSingleStepScheduler, "euler": S.EulerDiscreteScheduler,
          "euler_a": S.EulerAncestralDiscreteScheduler, "dpm": S.DPMSolverMultistepScheduler}[src]
    cfg = mk().config
    e = S.EulerDiscreteScheduler.from_config(cfg, use_karras_sigmas=True)
    assert e.use_karras_sigmas and e.config.use_karras_sigmas
    d = S.DPMSolverMultistepScheduler.from_config(cfg, use_karras_sigmas=True, algorithm_type="sde-dpmsolver++")
    assert d.use_karras_sigmas and d.config.algorithm_type == "sde-dpmsolver++" and d.config.solver_order == 2
    a = S.EulerAncestralDiscreteScheduler.from_config(cfg)
    for s in (e, d, a):
        assert s.config.steps_offset == cfg["steps_offset"] and s.config.timestep_spacing == cfg["timestep_spacing"]
    back = S.DDPMScheduler.from_config(d.config)       # keys of the other classes are ignored
    assert back.config.steps_offset == cfg["steps_offset"]
    lcm = S.LCMSingleStepScheduler.from_config(d.config)
    assert lcm.config.original_inference_steps == 50


def test_from_pretrained_reads_another_class_name(tmp_path):
    (tmp_path / "scheduler").mkdir()
    (tmp_path / "scheduler" / "scheduler_config.json").write_text(json.dumps(SDXL_CONFIG))
    d = S.DPMSolverMultistepScheduler.from_pretrained(str(tmp_path), subfolder="scheduler", use_karras_sigmas=True)
    assert d.use_karras_sigmas and d.config.timestep_spacing == "leading"
    e = S.EulerDiscreteScheduler.from_pretrained(str(tmp_path), subfolder="scheduler")
    e.set_timesteps(30)
    assert abs(e.init_noise_sigma - 11.5203) < 2e-4


@pytest.mark.parametrize("cls,key,val", [
    ("euler", "prediction_type", "v_prediction"), ("euler", "interpolation_type", "log_linear"),
    ("euler", "rescale_betas_zero_snr", True), ("euler", "timestep_spacing", "karras"),
    ("euler_a", "prediction_type", "v_prediction"), ("euler_a", "rescale_betas_zero_snr", True),
    ("euler_a", "interpolation_type", "log_linear"),
    ("dpm", "algorithm_type", "dpmsolver"), ("dpm", "algorithm_type", "sde-dpmsolver"), ("dpm", "solver_order", 3),
    ("dpm", "solver_type", "heun"), ("dpm", "thresholding", True), ("dpm", "use_lu_lambdas", True),
    ("dpm", "final_sigmas_type", "sigma_min"), ("dpm", "prediction_type", "v_prediction"),
    ("dpm", "rescale_betas_zero_snr", True)])
def test_refused_options_name_the_key(cls, key, val):
    C = {"euler": S.EulerDiscreteScheduler, "euler_a": S.EulerAncestralDiscreteScheduler, "dpm": S.DPMSolverMultistepScheduler}[cls]
    with pytest.raises(ValueError, match=key):
        C(**{key: val})
    with pytest.raises(ValueError, match=key):
        C.from_config(SDXL_CONFIG, **{key: val})


def test_s_churn_and_custom_timesteps_refused():
    e = S.EulerDiscreteScheduler()
    e.set_timesteps(4)
    with pytest.raises(ValueError, match="s_churn"):
        e.step(torch.zeros(1), e.timesteps[0], torch.zeros(1), s_churn=0.5)
    for C in (S.EulerDiscreteScheduler, S.EulerAncestralDiscreteScheduler, S.DPMSolverMultistepScheduler):
        with pytest.raises(ValueError, match="timesteps"):
            C().set_timesteps(timesteps=[999, 500, 1])


def test_set_timesteps_resets_step_state():
    d = S.DPMSolverMultistepScheduler()
    d.set_timesteps(10)
    d._step_index, d._lower_order_nums, d._hist = 4, 2, torch.zeros(1)
    d.set_timesteps(10)
    assert d.step_index is None and d._lower_order_nums == 0 and d._hist is None
    assert d.index_for_timestep(d.timesteps[3]) == 3


# ---- C ABI: argument checks run before any HIP call ------------------------------------------------------------------------
def test_new_entries_reject_bad_arguments_without_a_gpu():
    from instantir_amd import lib
    h = lib.load()
    P = 4096
    f = ctypes.c_float
    # iir_pack_latent_dscale(x, B, C, HW, out, ldo, rep, scale*, dtype, stream)
    assert h.iir_pack_latent_dscale(None, 1, 4, 16, P, 8, 2, P, 0, None) == -1
    assert h.iir_pack_latent_dscale(P, 1, 4, 16, P, 8, 2, None, 0, None) == -1          # no device scale
    assert h.iir_pack_latent_dscale(P, 1, 4, 16, P, 3, 2, P, 0, None) == -1             # ldo < C
    assert h.iir_pack_latent_dscale(P, 1, 4, 16, P, 8, 0, P, 0, None) == -1             # rep
    assert h.iir_pack_latent_dscale(P, 0, 4, 16, P, 8, 1, P, 0, None) == -1             # B
    assert h.iir_pack_latent_dscale(P, 1, 4, 16, P, 8, 1, P, 7, None) == -1             # dtype
    # iir_sched_step on a descriptor with the HIST bit (the former iir_sched_step_hist)
    ok = dict(eps_nhwc=P, lde=8, B=1, C=4, HW=16, cfg=1, coef=P, groups=lib.STEP_HIST, x=P + 256, hist=P + 512, prev=P + 768)

    def call(**kw):
        return h.iir_sched_step(ctypes.byref(lib.SchedDesc(**dict(ok, **kw))), None)
    for bad in (dict(eps_nhwc=None), dict(coef=None), dict(x=None), dict(hist=None), dict(prev=None), dict(B=0), dict(C=0), dict(HW=0),
                dict(lde=3), dict(cfg=0, eps_factor=P), dict(hist=P + 256), dict(hist=P + 768), dict(x0_out=P + 512),
                dict(groups=0), dict(groups=lib.STEP_HIST | 256)):          # ... a hist without its bit, a bit outside the four
        assert call(**bad) == -1, bad
    # iir_sched_step_hist_f32(eps, x, noise, coef, hist, n, prev, x0_out, stream)
    assert h.iir_sched_step_hist_f32(None, P, None, P, P + 64, 8, P + 128, None, None) == -1
    assert h.iir_sched_step_hist_f32(P, P + 32, None, P, None, 8, P + 128, None, None) == -1
    assert h.iir_sched_step_hist_f32(P, P + 32, None, None, P + 64, 8, P + 128, None, None) == -1
    assert h.iir_sched_step_hist_f32(P, P + 32, None, P, P + 64, 0, P + 128, None, None) == -1
    assert h.iir_sched_step_hist_f32(P, P + 32, None, P, P + 32, 8, P + 128, None, None) == -1      # hist aliases x
    assert h.iir_sched_step_hist_f32(P, P + 32, None, P, P, 8, P + 128, None, None) == -1           # hist aliases eps
    assert h.iir_sched_step_hist_f32(P, P + 32, None, P, P + 64, 8, P + 64, None, None) == -1      # hist aliases prev
    assert h.iir_sched_step_hist_f32(P, P + 32, None, P, P + 64, 8, P + 128, P + 64, None) == -1   # hist aliases x0_out
    del f


# ---- CLI ----------------------------------------------------------------------------------------------------------------
def test_cli_scheduler_flags():
    from types import SimpleNamespace
    from instantir_amd.infer import apply_scheduler, build_parser
    p = build_parser()
    a = p.parse_args(["--test_path", "x"])
    assert a.scheduler == "ddpm" and a.karras is False
    a = p.parse_args(["--test_path", "x", "--scheduler", "dpmpp_2m", "--karras"])
    assert a.scheduler == "dpmpp_2m" and a.karras
    with pytest.raises(SystemExit):
        p.parse_args(["--test_path", "x", "--scheduler", "lms"])
    pipe = SimpleNamespace(scheduler=S.DDPMScheduler())
    ddpm = pipe.scheduler
    apply_scheduler(pipe, a)
    assert type(pipe.scheduler) is S.DPMSolverMultistepScheduler and pipe.scheduler.use_karras_sigmas
    assert pipe.scheduler.config.algorithm_type == "dpmsolver++"
    for name, cls, algo in [("euler", S.EulerDiscreteScheduler, None), ("euler_a", S.EulerAncestralDiscreteScheduler, None),
                            ("dpmpp_2m_sde", S.DPMSolverMultistepScheduler, "sde-dpmsolver++"), ("ddim", S.DDIMScheduler, None)]:
        pipe = SimpleNamespace(scheduler=S.DDPMScheduler())
        apply_scheduler(pipe, p.parse_args(["--test_path", "x", "--scheduler", name]))
        assert type(pipe.scheduler) is cls and (algo is None or pipe.scheduler.config.algorithm_type == algo)
    pipe = SimpleNamespace(scheduler=ddpm)
    apply_scheduler(pipe, p.parse_args(["--test_path", "x"]))
    assert pipe.scheduler is ddpm                                       # the default leaves the pipeline as built
    with pytest.raises(SystemExit):
        apply_scheduler(pipe, p.parse_args(["--test_path", "x", "--scheduler", "euler_a", "--karras"]))
