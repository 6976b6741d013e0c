"""Noise schedulers of the InstantIR path, MI355X host side.

Host logic (integer timetables, fp32 coefficient tables) is plain Python/torch-CPU; tensor updates
run through the HIP kernels `iir_sched_step_f32` / `iir_axpby_f32` / `iir_lcm_step` and, inside the
denoising loop, fused with classifier-free guidance in `iir_sched_step`.

API mirrors what `pipelines/sdxl_instantir.py` touches on a scheduler object:
`set_timesteps`, `timesteps`, `config.{steps_offset,num_train_timesteps}`, `order`,
`init_noise_sigma`, `scale_model_input`, `add_noise`, `step(...) -> .prev_sample /
.pred_original_sample`, `alphas_cumprod`, `from_config`.

* `LCMSingleStepScheduler`: schedulers/lcm_single_step_scheduler.py:194-249 (tables), :331-399
  (set_timesteps and its ValueErrors), :401-407, :421-489 (step), :492-513 (add_noise).
* `DDPMScheduler` / `DDIMScheduler`: diffusers-0.28.1 classes constructed at infer.py:137 from SDXL's
  scheduler_config.json: scaled_linear betas 0.00085..0.012, 1000 train
  steps, steps_offset 1, "leading" spacing, epsilon prediction, fixed_small variance, no clipping.
* `EulerDiscreteScheduler` / `EulerAncestralDiscreteScheduler` / `DPMSolverMultistepScheduler`: the diffusers-0.28.1 classes a
  user swaps in with `Cls.from_config(pipe.scheduler.config)` (the reference's loop calls `scale_model_input`,
  pipelines/sdxl_instantir.py:1503-1504).  Epsilon prediction; the options each class refuses raise ValueError naming the key.
  `loop_coefficients(i)` drives the captured loop (`iir_pack_latent_dscale` + `iir_sched_step` with IIR_STEP_HIST).
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import List, Optional

import numpy as np
import torch


class _Config(dict):
    __getattr__ = dict.__getitem__


class SchedulerOutput(SimpleNamespace):
    """`.prev_sample`, `.pred_original_sample` (and `.denoised` for the LCM scheduler)."""

    def __getitem__(self, i):
        return tuple(self.__dict__.values())[i]


_SDXL_DEFAULTS = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                      steps_offset=1, timestep_spacing="leading", prediction_type="epsilon", clip_sample=False,
                      set_alpha_to_one=False)


def _alphas_cumprod(num_train_timesteps, beta_start, beta_end, beta_schedule):
    if beta_schedule == "scaled_linear":
        betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
    elif beta_schedule == "linear":
        betas = torch.linspace(beta_start, beta_end, num_train_timesteps, dtype=torch.float32)
    else:
        raise NotImplementedError(f"{beta_schedule} does is not implemented")
    return torch.cumprod(1.0 - betas, dim=0), betas


def _dev_coef(vals, device):
    return torch.tensor(vals, dtype=torch.float32).to(device)


def _custom_timetable(num_inference_steps, timesteps, T):
    """A caller's own descending `timesteps` as int64, checked; None when `num_inference_steps` sets the timetable."""
    if num_inference_steps is not None and timesteps is not None:
        raise ValueError("Can only pass one of `num_inference_steps` or `custom_timesteps`.")
    if timesteps is None:
        return None
    for i in range(1, len(timesteps)):
        if timesteps[i] >= timesteps[i - 1]:
            raise ValueError("`custom_timesteps` must be in descending order.")
    if timesteps[0] >= T:
        raise ValueError(f"`timesteps` must start before `self.config.train_timesteps`: {T}.")
    return np.array(timesteps, dtype=np.int64)


def _add_noise(original_samples, noise, pairs):
    """sa * x + sb * noise with one (sa, sb) pair per batch row.  CUDA fp32 tensors with one pair for every row go through
    the HIP kernel; anything else is computed with the same formula on its own device (host plumbing)."""
    if original_samples.is_cuda and original_samples.dtype == torch.float32 and all(p == pairs[0] for p in pairs):
        from . import ops
        out = torch.empty_like(original_samples)
        ops.axpby_f32(original_samples.contiguous(), noise.contiguous().float(), _dev_coef(list(pairs[0]), original_samples.device), out)
        return out
    shape = (-1,) + (1,) * (original_samples.dim() - 1)
    sa = torch.tensor([p[0] for p in pairs], dtype=original_samples.dtype, device=original_samples.device).reshape(shape)
    sb = torch.tensor([p[1] for p in pairs], dtype=original_samples.dtype, device=original_samples.device).reshape(shape)
    return sa * original_samples + sb * noise


def _run_step(model_output, sample, coef, generator=None, variance_noise=None, hist=None):
    """One `.step()` update on the GPU (iir_sched_step_f32 / iir_sched_step_hist_f32 with `hist`): (prev, x0) in the sample's
    dtype.  The noise is drawn here, fp32 on the generator's device, only when k_noise != 0 and none was given."""
    from . import ops
    noise = None
    if coef[6] != 0.0:
        if variance_noise is None:
            variance_noise = torch.randn(model_output.shape, generator=generator,
                                         device=generator.device if generator is not None else model_output.device,
                                         dtype=torch.float32)
        noise = variance_noise.float().contiguous().to(sample.device)
    x = sample.float().contiguous()
    e = model_output.float().contiguous()
    prev, x0 = torch.empty_like(x), torch.empty_like(x)
    ops.sched_step_f32(e, x, _dev_coef(coef, x.device), prev, noise=noise, x0_out=x0, hist=hist)
    return prev.to(sample.dtype), x0.to(sample.dtype)


class _Base:
    order = 1
    init_noise_sigma = 1.0

    def __init__(self, **kw):
        cfg = dict(_SDXL_DEFAULTS)
        cfg.update(kw)
        self.config = _Config(cfg)
        self.alphas_cumprod, self.betas = _alphas_cumprod(cfg["num_train_timesteps"], cfg["beta_start"], cfg["beta_end"],
                                                          cfg["beta_schedule"])
        self.final_alpha_cumprod = torch.tensor(1.0) if cfg.get("set_alpha_to_one", False) else self.alphas_cumprod[0]
        self.num_inference_steps = None
        self.timesteps = torch.from_numpy(np.arange(0, cfg["num_train_timesteps"])[::-1].copy().astype(np.int64))

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, subfolder=None, **kw):
        """`DDPMScheduler.from_pretrained(sdxl_path, subfolder="scheduler")` (infer.py:137): reads
        `<dir>[/<subfolder>]/scheduler_config.json`; local directories only."""
        import json
        import os
        d = os.path.join(pretrained_model_name_or_path, subfolder) if subfolder else pretrained_model_name_or_path
        path = os.path.join(d, "scheduler_config.json")
        if not os.path.isfile(path):
            raise FileNotFoundError(f"{path} not found (hub ids cannot be fetched: no network)")
        with open(path) as f:
            return cls.from_config(json.load(f), **kw)

    @classmethod
    def from_config(cls, config, **kw):
        """As diffusers: a config of any scheduler class; keys this class does not take are ignored, `kw` overrides."""
        import inspect
        names = set(_SDXL_DEFAULTS)
        for k in cls.__mro__:
            if "__init__" in vars(k):
                names |= set(inspect.signature(k.__init__).parameters) - {"self", "kw"}
        args = {k: v for k, v in dict(config).items() if k in names}
        args.update(kw)
        return cls(**args)

    def scale_model_input(self, sample, timestep=None):
        return sample

    def set_timesteps(self, num_inference_steps=None, device=None, timesteps: Optional[List[int]] = None):
        T = self.config.num_train_timesteps
        ts = _custom_timetable(num_inference_steps, timesteps, T)
        if ts is not None:
            self.custom_timesteps = True
            self.num_inference_steps = len(ts)
        else:
            if num_inference_steps > T:
                raise ValueError(f"`num_inference_steps`: {num_inference_steps} cannot be larger than "
                                 f"`self.config.train_timesteps`: {T}")
            self.num_inference_steps = num_inference_steps
            self.custom_timesteps = False
            # "leading": (i * floor(T/N))[::-1] + steps_offset, int64  
            step_ratio = T // num_inference_steps
            ts = (np.arange(0, num_inference_steps) * step_ratio).round()[::-1].copy().astype(np.int64)
            ts += self.config.steps_offset
        self.timesteps = torch.from_numpy(ts)
        if device is not None:
            self.timesteps = self.timesteps.to(device)

    def _prev_timestep(self, t):
        if getattr(self, "custom_timesteps", False):
            idx = (self.timesteps.cpu() == t).nonzero(as_tuple=True)[0][0]
            return -1 if idx == len(self.timesteps) - 1 else int(self.timesteps[idx + 1])
        n = self.num_inference_steps if self.num_inference_steps else self.config.num_train_timesteps
        return t - self.config.num_train_timesteps // n

    def add_noise(self, original_samples, noise, timesteps):
        """sqrt(abar_t) x + sqrt(1-abar_t) noise (the fp32 table's values), one t per batch row."""
        acp = self.alphas_cumprod
        t = torch.as_tensor(timesteps).reshape(-1).cpu().long()
        sa, sb = acp[t] ** 0.5, (1 - acp[t]) ** 0.5
        return _add_noise(original_samples, noise, list(zip(sa.tolist(), sb.tolist())))

    # coefficients of prev = k_x0*x0 + k_x*x + k_eps*eps + k_noise*noise, x0 = (x - sb*eps)/sa
    def step_coefficients(self, t, **kw):
        raise NotImplementedError

    def step(self, model_output, timestep, sample, eta=None, generator=None, variance_noise=None, return_dict=True, **kw):
        if not sample.is_cuda:
            raise RuntimeError("scheduler.step: tensors must live on the GPU (the update runs in the HIP library)")
        c = self.step_coefficients(int(timestep), eta=eta if eta is not None else 0.0)
        prev, x0 = _run_step(model_output, sample, c, generator, variance_noise)
        if not return_dict:
            return (prev,)
        return SchedulerOutput(prev_sample=prev, pred_original_sample=x0)


class DDPMScheduler(_Base):
    """Ancestral sampler used by infer.py:137.  variance_type fixed_small."""

    def step_coefficients(self, t, **kw):
        acp = self.alphas_cumprod
        prev_t = self._prev_timestep(t)
        a_t = acp[t]
        a_prev = acp[prev_t] if prev_t >= 0 else torch.tensor(1.0)
        b_t, b_prev = 1 - a_t, 1 - a_prev
        cur_alpha = a_t / a_prev
        cur_beta = 1 - cur_alpha
        k_x0 = (a_prev ** 0.5 * cur_beta) / b_t
        k_x = cur_alpha ** 0.5 * b_prev / b_t
        k_noise = torch.tensor(0.0)
        if t > 0:
            var = torch.clamp((1 - a_prev) / (1 - a_t) * cur_beta, min=1e-20)
            k_noise = var ** 0.5
        return [0.0, float(b_t ** 0.5), float(a_t ** 0.5), float(k_x0), float(k_x), 0.0, float(k_noise), 0.0]


class DDIMScheduler(_Base):
    """Deterministic (eta = 0) benchmark / parity default."""

    def step_coefficients(self, t, eta=0.0, **kw):
        acp = self.alphas_cumprod
        prev_t = self._prev_timestep(t)
        a_t = acp[t]
        a_prev = acp[prev_t] if prev_t >= 0 else self.final_alpha_cumprod
        b_t = 1 - a_t
        var = ((1 - a_prev) / (1 - a_t)) * (1 - a_t / a_prev)
        std = eta * var ** 0.5
        k_eps = (1 - a_prev - std ** 2) ** 0.5
        return [0.0, float(b_t ** 0.5), float(a_t ** 0.5), float(a_prev ** 0.5), 0.0, float(k_eps),
                float(std) if eta > 0 else 0.0, 0.0]


class LCMSingleStepScheduler(_Base):
    """One-step x0 preview with LCM boundary scalings; never touches `self.timesteps` in `step`."""

    def __init__(self, original_inference_steps: int = 50, timestep_scaling: float = 10.0, **kw):
        kw.setdefault("steps_offset", 0)
        kw.setdefault("set_alpha_to_one", True)
        super().__init__(**kw)
        self.config["original_inference_steps"] = original_inference_steps
        self.config["timestep_scaling"] = timestep_scaling
        self.sigma_data = 0.5

    def set_timesteps(self, num_inference_steps=None, device=None, original_inference_steps=None, strength=1.0,
                      timesteps=None):
        T = self.config.num_train_timesteps
        ts = _custom_timetable(num_inference_steps, timesteps, T)
        if ts is None:
            if num_inference_steps > T:
                raise ValueError(f"`num_inference_steps`: {num_inference_steps} cannot be larger than {T}")
            self.num_inference_steps = num_inference_steps
            orig = original_inference_steps if original_inference_steps is not None else self.config.original_inference_steps
            if orig > T:
                raise ValueError(f"`original_steps`: {orig} cannot be larger than {T}")
            if num_inference_steps > orig:
                raise ValueError(f"`num_inference_steps`: {num_inference_steps} cannot be larger than "
                                 f"`original_inference_steps`: {orig}")
            c = T // orig
            origin = np.asarray(list(range(1, int(orig * strength) + 1))) * c - 1
            skipping = len(origin) // num_inference_steps
            ts = origin[::-skipping][:num_inference_steps]
        self.timesteps = torch.from_numpy(np.asarray(ts).copy()).to(device=device, dtype=torch.long)

    def get_scalings_for_boundary_condition_discrete(self, timestep):
        st = timestep * self.config.timestep_scaling
        c_skip = self.sigma_data ** 2 / (st ** 2 + self.sigma_data ** 2)
        c_out = st / (st ** 2 + self.sigma_data ** 2) ** 0.5
        return c_skip, c_out

    def preview_coefficients(self, t):
        """{sqrt(1-abar_t), sqrt(abar_t), c_out, c_skip} in fp32, for iir_lcm_step."""
        tt = torch.tensor([int(t)], dtype=torch.int64)
        a = self.alphas_cumprod.gather(-1, tt)
        c_skip, c_out = self.get_scalings_for_boundary_condition_discrete(tt)
        return [float(torch.sqrt(1 - a)), float(torch.sqrt(a)), float(c_out), float(c_skip)]

    def step(self, model_output, timestep, sample, generator=None, return_dict=True):
        """denoised = c_out * x0 + c_skip * sample, on the GPU via the scheduler kernel:
        prev = k_x0*x0 + k_x*x with k_x0 = c_out, k_x = c_skip."""
        if not sample.is_cuda:
            raise RuntimeError("LCMSingleStepScheduler.step: tensors must live on the GPU")
        sb, sa, c_out, c_skip = self.preview_coefficients(int(timestep))
        out, _ = _run_step(model_output, sample, [0.0, sb, sa, c_out, c_skip, 0.0, 0.0, 0.0])
        if not return_dict:
            return (out,)
        return SchedulerOutput(denoised=out)


# ---- sigma-space schedulers (diffusers 0.28.1 EulerDiscreteScheduler, EulerAncestralDiscreteScheduler,
# DPMSolverMultistepScheduler; epsilon prediction) -------------------------------------------------------------------
#
# Every update of these schedulers is, in the scheduler's own sample space, the linear form of `_Base` plus one history
# term:  prev = k_x0*x0 + k_x*x + k_eps*eps + k_h*m_prev + k_noise*noise,  x0 = (x - sb*eps)/sa.  Host coefficients are
# formed in fp64 from the fp32 sigma table and rounded once to fp32; the tensor update runs in iir_sched_step (IIR_STEP_HIST) / iir_sched_step_hist_f32.

def _sigma_table(alphas_cumprod):
    """sigma(t) = sqrt((1 - abar_t) / abar_t) over the training steps, fp32 (as diffusers forms it), and its fp32 log."""
    s = (((1 - alphas_cumprod) / alphas_cumprod) ** 0.5).numpy().astype(np.float32)
    return s, np.log(s)


def _karras(sigma_max, sigma_min, n, rho=7.0):
    ramp = np.linspace(0, 1, n)
    max_inv, min_inv = sigma_max ** (1 / rho), sigma_min ** (1 / rho)
    return (max_inv + ramp * (min_inv - max_inv)) ** rho


def _sigma_to_t(sigma, log_sigmas):
    """Log-sigma interpolation of a sigma onto the (fractional) training-step axis, weight clipped to [0, 1]."""
    log_sigma = np.log(np.maximum(sigma, 1e-10))
    dists = log_sigma - log_sigmas[:, np.newaxis]
    low_idx = np.cumsum((dists >= 0), axis=0).argmax(axis=0).clip(max=log_sigmas.shape[0] - 2)
    high_idx = low_idx + 1
    low, high = log_sigmas[low_idx], log_sigmas[high_idx]
    w = np.clip((low - log_sigma) / (low - high), 0, 1)
    return ((1 - w) * low_idx + w * high_idx).reshape(np.shape(sigma))


def _refuse(key, value, why):
    raise ValueError(f"{key}={value!r} is not supported by this scheduler ({why})")


class _SigmaBase(_Base):
    """Shared host side of the three sigma schedulers: timetable + sigmas, step index, `loop_coefficients(i)` for the
    denoising loop and a stateful `.step()` over the HIP entry `iir_sched_step_hist_f32`."""

    _spacings = ("leading", "trailing", "linspace")

    def __init__(self, rescale_betas_zero_snr: bool = False, **kw):
        super().__init__(**kw)
        if self.config.prediction_type != "epsilon":
            _refuse("prediction_type", self.config.prediction_type, "epsilon prediction only")
        if rescale_betas_zero_snr:
            _refuse("rescale_betas_zero_snr", rescale_betas_zero_snr, "zero-SNR rescaling is not implemented")
        if self.config.timestep_spacing not in self._spacings:
            _refuse("timestep_spacing", self.config.timestep_spacing, f"one of {self._spacings}")
        self.config["rescale_betas_zero_snr"] = False
        self._sig_train, self._log_sig_train = _sigma_table(self.alphas_cumprod)
        self.sigmas = torch.from_numpy(np.concatenate([self._sig_train[::-1], [0.0]]).astype(np.float32))
        self._reset()

    def _reset(self):
        self._step_index = None
        self._hist = None
        self._lower_order_nums = 0

    @property
    def step_index(self):
        return self._step_index

    def index_for_timestep(self, timestep):
        """Position of `timestep` in `self.timesteps` (the second match if it repeats, as diffusers picks)."""
        t = float(torch.as_tensor(timestep).reshape(-1)[0])
        idx = (self.timesteps.cpu().double() == t).nonzero().flatten()
        if len(idx) == 0:
            raise ValueError(f"timestep {t} is not in the scheduler's timetable")
        return int(idx[1 if len(idx) > 1 else 0])

    def _index(self, timestep):
        return self._step_index if self._step_index is not None else self.index_for_timestep(timestep)

    def _begin_timesteps(self, num_inference_steps, timesteps, sigmas):
        """Shared opening of the sigma schedulers' set_timesteps: (num_train_timesteps, N, timestep_spacing)."""
        if timesteps is not None or sigmas is not None:
            raise ValueError(f"{type(self).__name__}: custom `timesteps` / `sigmas` are not supported; pass num_inference_steps")
        T, N = self.config.num_train_timesteps, int(num_inference_steps)
        if N > T or N < 1:
            raise ValueError(f"`num_inference_steps`: {N} must be in [1, {T}]")
        self.num_inference_steps = N
        return T, N, self.config.timestep_spacing

    def _set(self, timesteps, sigmas, device):
        self.timesteps = torch.from_numpy(np.asarray(timesteps)).to(device=device)
        self.sigmas = torch.from_numpy(np.asarray(sigmas, dtype=np.float32))
        self._reset()

    def c_in(self, i):
        return 1.0

    def add_noise(self, original_samples, noise, timesteps):
        """sa_i * x0 + sb_i * noise with the noise-level pair of each row's timestep (`_noise_pair`)."""
        ts = torch.as_tensor(timesteps).reshape(-1)
        return _add_noise(original_samples, noise, [self._noise_pair(self.index_for_timestep(t)) for t in ts])

    def loop_coefficients(self, i):
        """Step i of the denoising loop, run from step 0: c_in (UNet input scale), the UNet / Aggregator timestep (float),
        the LCM preview's integer timestep (`t.to(torch.int64)`, pipelines/sdxl_instantir.py:1557) and the fp32 update
        coefficients {0, sb, sa, k_x0, k_x, k_eps, k_noise, k_h} (coef[0] is the guidance slot the loop fills)."""
        t = float(self.timesteps[i])
        coef = [float(np.float32(v)) for v in self._coefficients64(i, self._order_at(i, i))]
        return dict(c_in=float(np.float32(self.c_in(i))), t=t, t_lcm=int(t), coef=coef)

    def _order_at(self, i, lower_order_nums):
        return 1

    def step(self, model_output, timestep, sample, generator=None, variance_noise=None, return_dict=True, s_churn=0.0, **kw):
        if s_churn and s_churn > 0:
            _refuse("s_churn", s_churn, "stochastic churn is not implemented")
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        if not sample.is_cuda:
            raise RuntimeError("scheduler.step: tensors must live on the GPU (the update runs in the HIP library)")
        if self._step_index is None:
            self._step_index = self.index_for_timestep(timestep)
        i = self._step_index
        c = [float(np.float32(v)) for v in self._coefficients64(i, self._order_at(i, self._lower_order_nums))]
        if self._hist is None or self._hist.shape != sample.shape or self._hist.device != sample.device:
            # never read on a first-order step (k_h == 0)
            self._hist = torch.empty(sample.shape, dtype=torch.float32, device=sample.device)
        prev, x0 = _run_step(model_output, sample, c, generator, variance_noise, hist=self._hist)
        self._step_index += 1
        self._lower_order_nums = min(self._lower_order_nums + 1, self.config.get("solver_order", 1))
        if not return_dict:
            return (prev,)
        return SchedulerOutput(prev_sample=prev, pred_original_sample=x0)


class _EulerBase(_SigmaBase):
    """Sample space VE: x = x0 + sigma * eps.  Shared timetable of EulerDiscreteScheduler and the ancestral variant."""

    _karras_ok = True

    def __init__(self, interpolation_type: str = "linear", use_karras_sigmas: bool = False, **kw):
        super().__init__(**kw)
        if interpolation_type != "linear":
            _refuse("interpolation_type", interpolation_type, "linear interpolation only")
        self.config["interpolation_type"] = interpolation_type
        self.use_karras_sigmas = bool(use_karras_sigmas) and self._karras_ok
        if self._karras_ok:
            self.config["use_karras_sigmas"] = self.use_karras_sigmas

    @property
    def init_noise_sigma(self):
        m = float(self.sigmas.max())
        return m if self.config.timestep_spacing in ("linspace", "trailing") else (m ** 2 + 1) ** 0.5

    def set_timesteps(self, num_inference_steps=None, device=None, timesteps=None, sigmas=None):
        T, N, sp = self._begin_timesteps(num_inference_steps, timesteps, sigmas)
        if sp == "linspace":
            ts = np.linspace(0, T - 1, N, dtype=np.float32)[::-1].copy()
        elif sp == "leading":
            ts = (np.arange(0, N) * (T // N)).round()[::-1].copy().astype(np.float32)
            ts += self.config.steps_offset
        else:
            ts = np.arange(T, 0, -T / N).round().copy().astype(np.float32)
            ts -= 1
        sig = np.interp(ts, np.arange(0, len(self._sig_train)), self._sig_train)
        if self.use_karras_sigmas:
            sig = _karras(sig[0].item(), sig[-1].item(), N)
            ts = np.array([_sigma_to_t(s, self._log_sig_train) for s in sig])
        self._set(np.asarray(ts).astype(np.float32), np.concatenate([sig, [0.0]]).astype(np.float32), device)

    def c_in(self, i):
        s = float(self.sigmas[i])
        return 1.0 / (s * s + 1) ** 0.5

    def scale_model_input(self, sample, timestep=None):
        """x / sqrt(sigma_i^2 + 1)."""
        s = float(self.sigmas[self._index(timestep)])
        return sample / ((s * s + 1) ** 0.5)

    def _noise_pair(self, i):
        return 1.0, float(self.sigmas[i])


class EulerDiscreteScheduler(_EulerBase):
    """x' = x + (sigma_{i+1} - sigma_i) * eps; x0 = x - sigma_i * eps."""

    def _coefficients64(self, i, order):
        s, sn = float(self.sigmas[i]), float(self.sigmas[i + 1])
        return [0.0, s, 1.0, 0.0, 1.0, sn - s, 0.0, 0.0]


class EulerAncestralDiscreteScheduler(_EulerBase):
    """x' = x + (sigma_down - sigma_i) * eps + sigma_up * noise (no Karras sigmas in this class, as in diffusers 0.28)."""

    _karras_ok = False

    def _coefficients64(self, i, order):
        s, sn = float(self.sigmas[i]), float(self.sigmas[i + 1])
        up = (sn ** 2 * (s ** 2 - sn ** 2) / s ** 2) ** 0.5
        down = (sn ** 2 - up ** 2) ** 0.5
        return [0.0, s, 1.0, 0.0, 1.0, down - s, up, 0.0]


class DPMSolverMultistepScheduler(_SigmaBase):
    """DPM-Solver++ (2M, 2M SDE) in VP space: x = alpha_i * x0 + s_i * eps with alpha_i = 1/sqrt(sigma_i^2+1),
    s_i = sigma_i * alpha_i.  init_noise_sigma = 1 and scale_model_input is the identity.  Bare construction takes this
    project's SDXL defaults ("leading", steps_offset 1), as the other classes here do."""

    def __init__(self, solver_order: int = 2, algorithm_type: str = "dpmsolver++", solver_type: str = "midpoint",
                 lower_order_final: bool = True, euler_at_final: bool = False, use_karras_sigmas: bool = False,
                 use_lu_lambdas: bool = False, final_sigmas_type: str = "zero", thresholding: bool = False,
                 variance_type=None, **kw):
        super().__init__(**kw)
        if algorithm_type not in ("dpmsolver++", "sde-dpmsolver++"):
            _refuse("algorithm_type", algorithm_type, "dpmsolver++ or sde-dpmsolver++")
        if solver_order not in (1, 2):
            _refuse("solver_order", solver_order, "orders 1 and 2")
        if solver_type != "midpoint":
            _refuse("solver_type", solver_type, "the midpoint form only")
        if thresholding:
            _refuse("thresholding", thresholding, "dynamic thresholding is not implemented")
        if use_lu_lambdas:
            _refuse("use_lu_lambdas", use_lu_lambdas, "uniform-logSNR steps are not implemented")
        if final_sigmas_type != "zero":
            _refuse("final_sigmas_type", final_sigmas_type, "the final sigma is 0")
        if variance_type is not None:
            _refuse("variance_type", variance_type, "learned variance is not implemented")
        self.config.update(solver_order=solver_order, algorithm_type=algorithm_type, solver_type=solver_type,
                           lower_order_final=lower_order_final, euler_at_final=euler_at_final,
                           use_karras_sigmas=bool(use_karras_sigmas), use_lu_lambdas=False, final_sigmas_type="zero",
                           thresholding=False, variance_type=None)
        self.use_karras_sigmas = bool(use_karras_sigmas)

    @property
    def order(self):
        return self.config.solver_order

    def set_timesteps(self, num_inference_steps=None, device=None, timesteps=None, sigmas=None):
        T, N, sp = self._begin_timesteps(num_inference_steps, timesteps, sigmas)
        if sp == "linspace":
            ts = np.linspace(0, T - 1, N + 1).round()[::-1][:-1].copy().astype(np.int64)
        elif sp == "leading":
            ts = (np.arange(0, N + 1) * (T // (N + 1))).round()[::-1][:-1].copy().astype(np.int64)
            ts += self.config.steps_offset
        else:
            ts = np.arange(T, 0, -T / N).round().copy().astype(np.int64)
            ts -= 1
        if self.use_karras_sigmas:
            sig = _karras(float(self._sig_train[-1]), float(self._sig_train[0]), N)
            ts = np.array([_sigma_to_t(s, self._log_sig_train) for s in sig]).round().astype(np.int64)
            if len(np.unique(ts)) != len(ts):
                raise ValueError(f"use_karras_sigmas with num_inference_steps={N} gives repeated integer timesteps {ts.tolist()}")
        else:
            sig = np.interp(ts, np.arange(0, len(self._sig_train)), self._sig_train)
        self._set(ts, np.concatenate([sig, [0.0]]).astype(np.float32), device)

    def _noise_pair(self, i):
        s = float(self.sigmas[i])
        a = 1.0 / (s * s + 1) ** 0.5
        return a, s * a

    def _order_at(self, i, lower_order_nums):
        N = len(self.timesteps)
        cfg = self.config
        last_low = i == N - 1 and (cfg.euler_at_final or (cfg.lower_order_final and N < 15) or cfg.final_sigmas_type == "zero")
        if cfg.solver_order == 1 or lower_order_nums < 1 or last_low:
            return 1
        return 2

    def _coefficients64(self, i, order):
        s, sn = float(self.sigmas[i]), float(self.sigmas[i + 1])
        a, an = 1.0 / (s * s + 1) ** 0.5, 1.0 / (sn * sn + 1) ** 0.5
        sb, snb = s * a, sn * an
        if sn == 0.0:                           # final sigma 0: the step returns the data prediction x0
            return [0.0, sb, a, 1.0, 0.0, 0.0, 0.0, 0.0]
        emh = sn / s                            # e^(-h), h = log(sigma_i / sigma_{i+1})
        sde = self.config.algorithm_type == "sde-dpmsolver++"
        if sde:
            k_x, base, k_noise = (snb / sb) * emh, an * (1.0 - emh * emh), snb * (1.0 - emh * emh) ** 0.5
        else:
            k_x, base, k_noise = snb / sb, -an * (emh - 1.0), 0.0
        if order == 1:
            return [0.0, sb, a, base, k_x, 0.0, k_noise, 0.0]
        sp = float(self.sigmas[i - 1])
        r = np.log(sp / s) / np.log(s / sn)     # h_prev / h
        return [0.0, sb, a, base * (1.0 + 1.0 / (2.0 * r)), k_x, 0.0, k_noise, -base / (2.0 * r)]
