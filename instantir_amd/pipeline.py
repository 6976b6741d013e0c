"""`InstantIRPipeline` for MI355X: the reference's pipeline API over the HIP engine.

Mirrors `pipelines/sdxl_instantir.py::InstantIRPipeline` (constructor :303-348, `prepare_previewers`
:350-397, `__call__` :1065-1739) for the denoising path: same keyword arguments and defaults, same
error conventions for the checks it implements, same outputs.  The hot loop (:1497-1660) runs as
HIP kernel launches, optionally replayed from a hipGraph per loop phase.

Observable deviations, all documented in SURVEY.md Appendix C and DESIGN.md:
  Q2  a step whose cond_scale is <= 0.1 everywhere skips previewer and Aggregator and, as the reference's statements do
      (:1602-1603 run unconditionally), re-scales the PREVIOUS step's already scaled residuals (loop phase `unet_res`); the
      adds are skipped only when that compound scale is zero for every image (same result).  On step 0 there are no previous
      residuals: a clear error instead of the reference's NameError.
  callback_on_step_end may return `latents` and `prompt_embeds` (:1651-1659); a replaced context re-hoists the text K / V of the
      cross-attention blocks and re-captures the step.  `negative_prompt_embeds` is accepted and, as in the reference (the name
      is never read after the CFG concat at :1465), has no effect.
  Q3  preview latents are copied to the host only when `save_preview_row=True`.
  Q5  `multistep_restore=True` raises NotImplementedError (unusable with the shipped scheduler).
  Q8/Q13  Resampler / embeddings hoisted out of the step.
  Q15 the reference defaults `ip_adapter_image` to `[image]` BEFORE `check_inputs` (:1278-1279), so passing
      `ip_adapter_image_embeds` always trips its own "provide either ... or ..." check (:850-853); here the default is
      applied only when no embeds are given, so the embeds path (the parity hook) is usable.
Latents are carried in fp32 between steps (the reference carries fp16); UNet inputs are fp16.
Guidance additions the reference does not have: perturbed-attention guidance (`enable_pag`), adaptive
projected guidance (`enable_apg`) and smoothed-energy guidance (`enable_seg`, `seg_scale`: the perturbed rows of PAG with their
queries Gaussian-blurred over the token grid instead of an identity attention map; PAG and SEG exclude each other).
"""
from __future__ import annotations

import dataclasses
import math
import os
from types import SimpleNamespace
from typing import Callable, Dict, List, Optional, Union

import torch

from . import ops, pag, seg
from . import restore_map as rmap
from .config import UNetConfig, VAEConfig
from .engine import CPAD, F16, HipAggregator, HipUNet
from .schedulers import (DDIMScheduler, DDPMScheduler, DPMSolverMultistepScheduler, EulerAncestralDiscreteScheduler,  # noqa: F401
                         EulerDiscreteScheduler, LCMSingleStepScheduler)
from .weights import LCM_LORA_MODULES, PREVIEWER_LORA_MODULES, aggregator_specs, lora_target

COLOR_FIX_MODES = (None,) + ops.COLOR_FIX_MODES          # `color_fix=` of __call__ / restore_single_step


def _tokenizer_fn(tk):
    """A transformers tokenizer as the callable the pipeline holds: list[str] -> (B, 77) int64 ids, padded / truncated."""
    return lambda texts: tk(texts, padding="max_length", max_length=tk.model_max_length, truncation=True, return_tensors="pt").input_ids


def _clip_text(tensors, config, default_act, device):
    """`encoders.HipCLIPText` from a text encoder's tensors and its config.json mapping (None / {}: the architecture's defaults)."""
    from .encoders import HipCLIPText
    c = config or {}
    return HipCLIPText(tensors, device, hidden_act=c.get("hidden_act", default_act), eos_token_id=c.get("eos_token_id", 2),
                       eps=c.get("layer_norm_eps", 1e-5))


def _image_array(images, same_size=None):
    """PIL / numpy image(s) -> fp32 NCHW tensor in [0, 1].  `same_size`: what to call the images when their sizes differ."""
    import numpy as np
    if not isinstance(images, (list, tuple)):
        images = [images]
    arrs = [np.asarray(im.convert("RGB") if hasattr(im, "convert") else im, dtype=np.float32) / 255.0 for im in images]
    if same_size is not None and len({a.shape for a in arrs}) != 1:
        raise ValueError(f"{same_size} images must share one size")
    return torch.from_numpy(np.stack(arrs)).permute(0, 3, 1, 2)


def _randn(shape, generator, device):
    """fp32 normal draw on the generator's own device (a host generator draws on the host), on `device` without one."""
    return torch.randn(tuple(shape), generator=generator, device=generator.device if generator is not None else device, dtype=torch.float32)


def _time_ids(rows, n):
    """`add_time_ids` rows (original size + crop offset + target size, :965-981), the block repeated `n` times."""
    return torch.tensor(rows, dtype=torch.float32).repeat(n, 1)


class StableDiffusionXLPipelineOutput(SimpleNamespace):
    """`.images` like diffusers' output class (pipelines/sdxl_instantir.py:1739)."""


class _AggregatorHandle:
    """`pipe.aggregator.load_state_dict(sd)` / `.to(...)` surface of infer.py:142-144."""

    def __init__(self, pipe):
        self._pipe = pipe

    def load_state_dict(self, sd, strict=True):
        k = "controlnet_mid_block.0.mlp_shared.0.weight"            # SFT hidden width comes from the file (module/aggregator.py:60)
        if k in sd and sd[k].shape[0] != self._pipe.cfg.sft_hidden:
            self._pipe.cfg = dataclasses.replace(self._pipe.cfg, sft_hidden=sd[k].shape[0])
        want = {n for n, _, _ in aggregator_specs(self._pipe.cfg)}
        missing, unexpected = sorted(want - set(sd)), sorted(set(sd) - want)
        if strict and (missing or unexpected):
            raise RuntimeError(f"Error(s) in loading state_dict for Aggregator: missing {missing[:5]} unexpected {unexpected[:5]}")
        self._pipe._agg_sd = dict(sd)
        self._pipe._agg = None
        self._pipe._loop_cache = None               # (the entry pins the released engine)

    def to(self, *a, **k):
        return self

    def from_unet(self):
        """`Aggregator.from_unet(unet)` + `remove_attn2` (module/aggregator.py:503-578, pipelines/sdxl_instantir.py:165-177,
        320-322) -- what the reference pipeline holds when no aggregator is passed in: `conv_in` (also as `ref_conv_in`),
        time / add embeddings, down blocks and mid block copied from the UNet (cross-attention and its norm dropped), the
        SFT heads freshly initialised behind zero 1x1 convolutions, so every residual it emits is exactly zero.  (The
        reference draws the SFT 3x3 weights from PyTorch's default init; behind the zero convs their values are unobservable,
        zeros are used.)"""
        usd = self._pipe._unet_sd
        out = {}
        for name, shape, _ in aggregator_specs(self._pipe.cfg):
            if name.startswith("ref_conv_in."):
                out[name] = usd["conv_in." + name[len("ref_conv_in."):]]
            elif name.startswith("controlnet_"):
                out[name] = torch.zeros(shape, dtype=torch.float32)
            else:
                out[name] = usd[name]
        return out


class _UNetHandle:
    """The slice of `pipe.unet`'s peft surface the reference's callers touch: `set_adapter` / `active_adapters`
    (gradio_demo/app.py:116-120 switches between the `previewer` and `lcm` LoRAs per request), `enable_adapters` /
    `disable_adapters` (pipelines/sdxl_instantir.py:396, :1543, :1556).  Each adapter is a merged second weight copy built on
    first use and kept (5 GB at SDXL size); switching adapters swaps which copy the previewer pass launches."""

    def __init__(self, pipe):
        self._pipe = pipe

    def active_adapters(self):
        return [self._pipe._active_adapter] if self._pipe._active_adapter is not None else []

    def set_adapter(self, name):
        if isinstance(name, (list, tuple)):
            if len(name) != 1:
                raise ValueError("one active LoRA adapter at a time (the reference's callers never mix them)")
            name = name[0]
        if name not in self._pipe._adapters:
            raise ValueError(f"Adapter {name} not found. Available adapters: {list(self._pipe._adapters)}")
        self._pipe._active_adapter = name
        self._pipe._unet_prev = self._pipe._prev_nets.get((name, 1.0))
        self._pipe._loop_cache = None               # its entry pins the previewer copy it was captured on, switched away from or
        #                                             released by `prepare_previewers` (~5 GB at SDXL size)

    def enable_adapters(self):       # the loop itself decides which pass runs with the LoRA (:1543-1556)
        pass

    def enable_freeu(self, s1, s2, b1, b2):     # module/unet/unet_2d_ZeroSFT.py:919-943: the pipeline's switch, one state
        self._pipe.enable_freeu(s1, s2, b1, b2)

    def disable_freeu(self):                     # :945-949
        self._pipe.disable_freeu()

    def disable_adapters(self):
        pass


class InstantIRPipeline:
    vae_scale_factor = 8

    def __init__(self, cfg: UNetConfig, unet_state_dict: Dict[str, torch.Tensor], aggregator_state_dict=None,
                 scheduler=None, vae=None, device="cuda:0", image_encoder=None, text_encoder=None, text_encoder_2=None,
                 tokenizer=None, tokenizer_2=None):
        """unet_state_dict: diffusers SDXL names + TA-IP processor + Resampler weights (what
        `load_adapter_to_pipe` leaves in `pipe.unet`, module/ip_adapter/utils.py:136-161)."""
        self.cfg = cfg
        self.device = torch.device(device)
        self._unet_sd = unet_state_dict
        self._agg_sd = aggregator_state_dict
        self._adapters = {}                          # name -> (peft-named LoRA tensors, alpha / r)
        self._active_adapter = None
        self._prev_nets = {}                         # (adapter, cross_attention_kwargs["scale"]) -> merged previewer copy
        self.unet = _UNetHandle(self)
        self.scheduler = scheduler if scheduler is not None else DDPMScheduler()
        self.aggregator = _AggregatorHandle(self)
        self.vae = vae
        self.image_encoder = image_encoder          # encoders.HipDinov2 (module/ip_adapter/utils.py:106-118)
        self.text_encoder, self.text_encoder_2 = text_encoder, text_encoder_2     # encoders.HipCLIPText
        self.tokenizer, self.tokenizer_2 = tokenizer, tokenizer_2               # callables: list[str] -> (B,77) int64 ids
        self._unet = self._unet_prev = self._agg = self._unet_prev8 = None
        self._loop_cache = None                     # (key, _DenoiseLoop) of the last call: see _loop_for
        self._prompt_cache = {}                     # (token ids, encoders) -> (prompt_embeds, pooled): see encode_prompt
        self.use_graphs = True
        self.overlap_streams = True
        self.overlap_sft = True                     # shallow SFT heads beside the decoder's first up block
        self._guidance_scale = 7.0
        self._freeu = None                          # (s1, s2, b1, b2) or None: see enable_freeu
        self._pag_layers = None                     # perturbed-attention guidance: the layer list of enable_pag, or None
        self._pag_paths = None                      # ... and the main UNet's `attn1` paths it selects
        self._seg_layers = self._seg_paths = None   # smoothed-energy guidance: the same pair for enable_seg ...
        self._seg_sigma = None                      # ... and its blur sigma
        self._apg = None                            # adaptive projected guidance: (eta, norm_threshold, momentum) or None
        self._device_preprocess = False             # encode_image preprocesses PIL images on the device: enable_device_preprocess

    # ---- reference surface ----------------------------------------------------------------------
    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, torch_dtype=None, device="cuda:0", **kwargs):
        """`InstantIRPipeline.from_pretrained(sdxl_dir, torch_dtype=torch.float16)` (infer.py:117-120): reads the SDXL
        directory layout with this build's own readers -- `unet/`, `vae/`, `text_encoder(_2)/`
        safetensors (+ config.json), `tokenizer(_2)/`.  Local directories only: there is no hub access.  The TA-IP
        adapter, previewer LoRA and Aggregator are attached afterwards exactly as infer.py does
        (`loaders.load_adapter_to_pipe`, `prepare_previewers`, `aggregator.load_state_dict`).  Compute is fp16 with
        fp32 accumulation whatever `torch_dtype` says."""
        from . import loaders
        from .vae import HipVAE
        d = pretrained_model_name_or_path
        if not os.path.isdir(d):
            raise FileNotFoundError(f"{d!r} is not a local directory (hub ids cannot be fetched: no network)")
        cfg, vc = loaders.unet_config_from_dir(d), loaders.vae_config_from_dir(d)
        unet_sd = loaders.load_component(d, "unet")
        vae = HipVAE(vc, loaders.load_component(d, "vae"), device) if os.path.isdir(os.path.join(d, "vae")) else None
        enc, tok = [], []
        for sub, tsub, default_act in (("text_encoder", "tokenizer", "quick_gelu"), ("text_encoder_2", "tokenizer_2", "gelu")):
            e = t = None
            if os.path.isdir(os.path.join(d, sub)):
                cj = os.path.join(d, sub, "config.json")
                c = loaders._read_json(cj) if os.path.isfile(cj) else {}
                e = _clip_text(loaders.load_component(d, sub), c, default_act, device)
            if os.path.isdir(os.path.join(d, tsub)):
                from transformers import CLIPTokenizer
                t = _tokenizer_fn(CLIPTokenizer.from_pretrained(os.path.join(d, tsub)))
            enc.append(e)
            tok.append(t)
        return cls(cfg, unet_sd, scheduler=kwargs.get("scheduler"), vae=vae, device=device, text_encoder=enc[0],
                   text_encoder_2=enc[1], tokenizer=tok[0], tokenizer_2=tok[1])

    @classmethod
    def from_modules(cls, vae=None, text_encoder=None, text_encoder_2=None, tokenizer=None, tokenizer_2=None, unet=None, scheduler=None,
                     aggregator=None, force_zeros_for_empty_prompt=True, add_watermarker=None, feature_extractor=None,
                     image_encoder=None, device="cuda:0", unet_config=None, vae_config=None):
        """The reference's own constructor signature (pipelines/sdxl_instantir.py:303-322): build the pipeline from module OBJECTS
        somebody else loaded -- anything with `.state_dict()` (diffusers / transformers modules, or plain dicts of their
        tensors) and, where geometry is not implied by the tensors, a `.config` (mapping or attribute object; `unet_config=` /
        `vae_config=` override it).  `aggregator=None` = `Aggregator.from_unet(unet)` (:319-320); tokenizers may be transformers
        tokenizers or callables `list[str] -> (B, 77) ids`; `image_encoder` a `HipDinov2` / `HipCLIPVision` or a module of one
        of those architectures (DINOv2 unless its tensors say CLIP).  `add_watermarker` / `feature_extractor` are accepted and
        unused (no watermarking; image pre-processing is `encoders.preprocess_*`), `force_zeros_for_empty_prompt` must stay True
        (the only value the reference's loaders produce)."""
        from . import loaders
        from .encoders import HipCLIPText, HipCLIPVision, HipDinov2
        from .vae import HipVAE
        if unet is None:
            raise ValueError("from_modules: `unet` is required")
        if not force_zeros_for_empty_prompt:
            raise NotImplementedError("force_zeros_for_empty_prompt=False is not supported")

        def tensors(m):
            return dict(m) if isinstance(m, dict) else dict(m.state_dict())

        def as_dict(c):
            if c is None:
                return None
            if hasattr(c, "keys"):
                return dict(c)
            if hasattr(c, "to_dict"):                                      # transformers PretrainedConfig
                return c.to_dict()
            return {k: getattr(c, k) for k in dir(c) if not k.startswith("_") and not callable(getattr(c, k))}

        def conf(m):
            return as_dict(getattr(m, "config", None))

        cfg = unet_config or (loaders.unet_config_from_dict(conf(unet)) if conf(unet) else UNetConfig.sdxl())
        hv = vae
        if vae is not None and not isinstance(vae, HipVAE):
            vc = vae_config or (loaders.vae_config_from_dict(conf(vae)) if conf(vae) else VAEConfig.sdxl())
            hv = HipVAE(vc, tensors(vae), device)
        encs = []
        for m, default_act in ((text_encoder, "quick_gelu"), (text_encoder_2, "gelu")):
            ready = m is None or isinstance(m, HipCLIPText)
            encs.append(m if ready else _clip_text(tensors(m), conf(m), default_act, device))
        # (a transformers tokenizer has `model_max_length`; anything else is taken as the ids callable itself)
        toks = [_tokenizer_fn(t) if t is not None and hasattr(t, "model_max_length") else t for t in (tokenizer, tokenizer_2)]
        ie = image_encoder
        if ie is not None and not isinstance(ie, (HipDinov2, HipCLIPVision)):
            sd_ie = tensors(ie)
            is_clip = any("vision_model" in k for k in sd_ie)
            c = conf(ie)
            if c is not None and c.get("vision_config") is not None:       # a CLIPConfig: the tower's own part
                c = as_dict(c["vision_config"])
            if c is None:                                                  # no config: the architectures' defaults
                kw = {}
            else:                                                          # (a ViT-H / bigG tower is not D // 64 heads)
                kw = {"num_heads": c.get("num_attention_heads"), "patch_size": c.get("patch_size", None if is_clip else 14),
                      "eps": c.get("layer_norm_eps", 1e-5 if is_clip else 1e-6)}
                if is_clip:
                    kw["hidden_act"] = c.get("hidden_act", "quick_gelu")
            ie = HipCLIPVision(sd_ie, device, **kw) if is_clip else HipDinov2(sd_ie, device, **kw)
        pipe = cls(cfg, tensors(unet), scheduler=scheduler, vae=hv, device=device, image_encoder=ie, text_encoder=encs[0],
                   text_encoder_2=encs[1], tokenizer=toks[0], tokenizer_2=toks[1])
        if aggregator is not None:
            pipe.aggregator.load_state_dict(tensors(aggregator))
        return pipe

    def to(self, *a, **k):
        return self

    @property
    def guidance_scale(self):
        return self._guidance_scale

    @property
    def _lora(self):
        return self._adapters[self._active_adapter][0] if self._active_adapter is not None else None

    @_lora.setter
    def _lora(self, v):            # bench.py drops the host copies once the device copies exist
        if v is None:
            self._adapters = {k: (None, sc) for k, (_, sc) in self._adapters.items()}

    @property
    def _lora_scaling(self):
        return self._adapters[self._active_adapter][1] if self._active_adapter is not None else 1.0

    def enable_freeu(self, s1, s2, b1, b2):
        """FreeU (diffusers' StableDiffusionMixin.enable_freeu -> module/unet/unet_2d_ZeroSFT.py:919-943): in up blocks 0 and
        1 the first half of the hidden channels is scaled by b1 / b2 and the skip goes through `fourier_filter` with scale
        s1 / s2 (module/min_sdxl.py:22-77) before each concat, in every UNet pass (main and previewer, and
        `restore_single_step`).  The up blocks test `s1 and s2 and b1 and b2` (unet_2d_ZeroSFT_blocks.py:2600-2605), so a
        zero factor switches FreeU off everywhere.  SDXL values from diffusers' docs: s1=0.9, s2=0.2, b1=1.3, b2=1.4."""
        f = tuple(float(v) for v in (s1, s2, b1, b2))
        self._freeu = f if all(f) else None

    def disable_freeu(self):
        self._freeu = None

    # ---- perturbed-attention guidance (PAG; behaviour of diffusers' PAG pipelines) ----
    def enable_pag(self, pag_applied_layers: Union[str, List[str]] = "mid"):
        """Turn PAG on for later calls (`pag_scale`, default 3.0; `pag_adaptive_scale`).  Each entry of `pag_applied_layers` is a
        regular expression over the main UNet's self-attention module names (e.g. 'mid', 'down_blocks.2', 'up_blocks.0',
        'up_blocks.1.attentions.2'); see `instantir_amd.pag.select`."""
        if self._seg_layers is not None:
            raise ValueError("enable_pag: smoothed-energy guidance is enabled and both methods claim the one perturbed row group; "
                             "call pipe.disable_seg() first")
        if self._unet is not None:
            pag.check_engine(self._unet)
        self.set_pag_applied_layers(pag_applied_layers)

    def set_pag_applied_layers(self, pag_applied_layers: Union[str, List[str]]):
        layers = pag.normalize_layers(pag_applied_layers)
        self._pag_paths = tuple(pag.select(layers, pag.attn1_paths(self.cfg)))
        self._pag_layers = layers

    def disable_pag(self):
        self._pag_layers = self._pag_paths = None

    @property
    def pag_applied_layers(self):
        return None if self._pag_layers is None else list(self._pag_layers)

    # ---- smoothed-energy guidance (SEG; Hong 2024) ----
    def enable_seg(self, seg_applied_layers: Union[str, List[str]] = "mid", seg_blur_sigma: float = seg.DEFAULT_SEG_BLUR_SIGMA):
        """Turn SEG on for later calls (`seg_scale`, default 3.0): the main UNet runs one more row group whose queries, in the
        self-attention layers `seg_applied_layers` selects (the expressions of `enable_pag`), are blurred over the token grid by a
        Gaussian of `seg_blur_sigma` (> 0; beyond 9999, `math.inf` included, the image's mean query), and the step adds
        seg_scale * (cond - perturbed).  Needs no prompt and no CFG.  PAG and SEG exclude each other."""
        if self._pag_layers is not None:
            raise ValueError("enable_seg: perturbed-attention guidance is enabled and both methods claim the one perturbed row group; "
                             "call pipe.disable_pag() first")
        if self._unet is not None:
            seg.check_engine(self._unet)
        sigma = seg.check_sigma(seg_blur_sigma)
        self.set_seg_applied_layers(seg_applied_layers)
        self._seg_sigma = sigma

    def set_seg_applied_layers(self, seg_applied_layers: Union[str, List[str]]):
        layers = pag.normalize_layers(seg_applied_layers, "seg_applied_layers")
        self._seg_paths = tuple(seg.select(layers, self.cfg))
        self._seg_layers = layers
        if self._seg_sigma is None:
            self._seg_sigma = seg.DEFAULT_SEG_BLUR_SIGMA

    def disable_seg(self):
        self._seg_layers = self._seg_paths = self._seg_sigma = None

    @property
    def seg_applied_layers(self):
        return None if self._seg_layers is None else list(self._seg_layers)

    @property
    def seg_blur_sigma(self):
        return self._seg_sigma

    # ---- adaptive projected guidance (APG; Sadat et al. 2024) ----
    def enable_apg(self, eta: float = 0.0, norm_threshold: float = 15.0, momentum: float = -0.5):
        """Turn adaptive projected guidance on for later calls: the CFG update, formed on denoised predictions, is split into its
        parts parallel and orthogonal to the cond prediction; the parallel part (which drives saturation) is weighted by `eta`
        (0 <= eta <= 1), the update's per-image norm is clamped to `norm_threshold` (>= 0; 0 = no clamp) and it carries a running
        average over the steps of a call with weight `momentum` (-1 < momentum < 1).  The defaults are this project's choice
        (DESIGN.md).  Calls then need guidance_scale > 1 and guidance_rescale == 0."""
        try:
            f = tuple(float(v) for v in (eta, norm_threshold, momentum))
        except (TypeError, ValueError):
            raise ValueError(f"enable_apg: eta, norm_threshold and momentum must be numbers, got {(eta, norm_threshold, momentum)!r}")
        if not all(math.isfinite(v) for v in f):
            raise ValueError(f"enable_apg: eta, norm_threshold and momentum must be finite, got {f}")
        if not 0.0 <= f[0] <= 1.0:
            raise ValueError(f"enable_apg: eta must be in [0, 1], got {f[0]}")
        if f[1] < 0.0:
            raise ValueError(f"enable_apg: norm_threshold must be >= 0 (0 = no clamp), got {f[1]}")
        if not -1.0 < f[2] < 1.0:
            raise ValueError(f"enable_apg: momentum must be in (-1, 1), got {f[2]}")
        self._apg = f

    def disable_apg(self):
        self._apg = None

    @property
    def apg(self):
        """(eta, norm_threshold, momentum) of `enable_apg`, or None."""
        return self._apg

    def _main_state(self, ctx, pooled, time_ids, img, Hl, Wl, B, rep, pag_on):
        """`prepare` of the main UNet: with PAG or SEG (`pag_on`) one more group of B rows, each a copy of its cond row (rows [(rep-1)B, rep B)
        of the prompt embeddings, pooled embeddings, time ids and IP tokens)."""
        ip = self._unet.resampler(img)
        if pag_on:
            c = slice((rep - 1) * B, rep * B)
            ctx, pooled, time_ids, ip = (torch.cat([v, v[c]], 0) for v in (ctx, pooled, time_ids, ip))
        return self._unet.prepare(ctx, pooled, time_ids, ip, Hl, Wl)

    def _apply_freeu(self, *nets):
        for n in nets:
            if n is not None:
                n.freeu = self._freeu

    @property
    def do_classifier_free_guidance(self):
        # pipelines/sdxl_instantir.py:1050-1051 (time_cond_proj_dim is None for SDXL)
        return self._guidance_scale > 1

    def prepare_previewers(self, lora_state_dict: Dict[str, torch.Tensor], use_lcm=False, lora_alpha=None):
        """pipelines/sdxl_instantir.py:350-397.  `lora_state_dict` holds peft-named tensors
        (`<module>.lora_A.weight` / `.lora_B.weight`) -- the form the reference has after
        `convert_unet_state_dict_to_peft` and the `attn2` -> `attn2.processor` rename (:364-370).
        Raises ValueError on keys that match no LoRA target (:390-394); missing keys are ignored."""
        targets = LCM_LORA_MODULES if use_lcm else PREVIEWER_LORA_MODULES
        if isinstance(lora_state_dict, (str, os.PathLike)):          # the reference's own call form: a directory / file path
            from .loaders import read_previewer_lora
            lora_state_dict, file_alpha = read_previewer_lora(os.fspath(lora_state_dict))
            lora_alpha = file_alpha if lora_alpha is None else lora_alpha
        ranks = {v.shape[0] for k, v in lora_state_dict.items() if k.endswith(".lora_A.weight")}
        if len(ranks) == 1 and next(iter(ranks)) != self.cfg.lora_rank:
            self.cfg = dataclasses.replace(self.cfg, lora_rank=next(iter(ranks)))
        unexpected = []
        for k in lora_state_dict:
            for suf in (".lora_A.weight", ".lora_B.weight"):
                if k.endswith(suf):
                    path = k[: -len(suf)]
                    if not lora_target(path, targets) or (path + ".weight") not in self._unet_sd:
                        unexpected.append(k)
                    break
            else:
                unexpected.append(k)
        if unexpected:
            raise ValueError("Loading adapter weights from state_dict led to unexpected keys not found in the model: "
                             f" {unexpected}. ")
        lora_alpha = 1 if lora_alpha is None else lora_alpha
        name = "lcm" if use_lcm else "previewer"                       # :383
        self._adapters[name] = (dict(lora_state_dict), lora_alpha / self.cfg.lora_rank)   # peft: alpha / r with r = 64 (:376-381)
        for k in [k for k in self._prev_nets if k[0] == name]:
            del self._prev_nets[k]
        self._unet_prev8 = None
        self.unet.set_adapter(name)        # diffusers' `add_adapter` ends in `set_adapter(adapter_name)`: the newest one is active
        return lora_alpha

    # ---- engine construction ----------------------------------------------------------------------
    def _build(self, lora_mult: float = 1.0):
        """`lora_mult`: `cross_attention_kwargs["scale"]`, which diffusers' UNet forward turns into `scale_lora_layers(unet, scale)`
        for the pass that runs with the adapters on -- i.e. the previewer copy is W + scale * (alpha / r) * B A."""
        if self._unet is None:
            self._unet = HipUNet(self.cfg, self._unet_sd, self.device)
        if self._active_adapter is not None:
            key = (self._active_adapter, float(lora_mult))
            if key not in self._prev_nets:
                self._loop_cache = None    # a new copy follows: the cached loop pins the one it replaces
                if float(lora_mult) != 1.0:
                    # a merged copy is a whole UNet (~5 GB at SDXL size): keep ONE non-default scale per adapter, evict the previous
                    for k_old in [k for k in self._prev_nets if k[0] == self._active_adapter and k[1] != 1.0 and len(k) == 2]:
                        del self._prev_nets[k_old]
                if self._lora is None:
                    raise RuntimeError(f"LoRA adapter {self._active_adapter!r}: the host copy was released; call prepare_previewers again")
                self._prev_nets[key] = HipUNet(self.cfg, self._unet_sd, self.device, lora=self._lora,
                                               lora_scaling=self._lora_scaling * float(lora_mult))
            self._unet_prev = self._prev_nets[key]
        if self._agg is None:
            if self._agg_sd is None:
                self._agg_sd = self.aggregator.from_unet()
            self._agg = HipAggregator(self.cfg, self._agg_sd, self.device)
        self._apply_freeu(self._unet, self._unet_prev)

    def _loop_for(self, B, rep, Hl, Wl, st, st_prev, st_agg, lq, reference_latents, previewer_scheduler, guidance_rescale, pag_on=False,
                  fresh=False, keep=None, apg_on=False, seg_on=False):
        """The step's buffers and captured hipGraphs are kept from one call to the next: a second image of the same geometry,
        through the same engines, re-uses them (its hoisted K / V, embeddings and LQ latent are copied into the captured
        tensors) instead of paying the warm-up step, the capture and the graph instantiation again (~0.1 s of a 1.9 s call
        at 1024^2).  Anything the captured launches depend on is part of the key; `IIR_LOOP_CACHE=0` switches it off.
        `fresh` (a callback replaced the context in mid-call): a new loop beside the cached one, which stays as it is."""
        nets = (self._unet, self._unet_prev, self._agg)
        key = (B, rep, Hl, Wl, reference_latents is not None, float(guidance_rescale or 0.0), self.use_graphs, self.overlap_streams,
               self.overlap_sft, tuple(None if n is None else (id(n), n.arena_gen, n.inkernel_prefetch) for n in nets),
               self._freeu,           # the FreeU factors are launch arguments of the captured concats
               _sched_form(self.scheduler),   # the sigma schedulers launch the device-scale pack and the history step
               self._pag_paths if pag_on and not seg_on else None,   # PAG: row count and the identity launches (its scale is a device scalar)
               (self._seg_paths, self._seg_sigma) if seg_on else None,   # SEG: row count, the blur launches and their taps (likewise)
               keep is not None,      # a restore map: the step's last launch carries IIR_STEP_KEEP, on buffers only such a loop has
               bool(apg_on))          # APG: iir_apg_project + IIR_STEP_APG in the step (its three parameters travel in the scalar row)
        if not fresh:
            cached = self._loop_cache
            if cached is not None and cached[0] == key and os.environ.get("IIR_LOOP_CACHE", "1") != "0":
                if cached[1].adopt(st, st_prev, st_agg, lq, reference_latents, previewer_scheduler, keep=keep):
                    return cached[1]
            self._loop_cache = cached = None         # drop the old graphs before building the new ones
        loop = _DenoiseLoop(self, B, rep, Hl, Wl, st, st_prev, st_agg, lq, reference_latents, previewer_scheduler,
                            guidance_rescale=guidance_rescale, pag_on=pag_on, keep=keep, apg_on=apg_on)
        # the entry keeps the engines alive: `id()` in the key can then not be re-issued to a NEW engine (adapter switch, LoRA
        # scale change) while graphs captured on the old one's arena and weights are still cached
        if not fresh:
            self._loop_cache = (key, loop, nets)
        return loop

    # ---- input checks (pipelines/sdxl_instantir.py:749-864, the conditions that apply to tensor inputs) ----
    def check_inputs(self, prompt, prompt_embeds, negative_prompt_embeds, pooled_prompt_embeds, negative_pooled_prompt_embeds,
                     ip_adapter_image, ip_adapter_image_embeds, control_guidance_start, control_guidance_end,
                     callback_on_step_end_tensor_inputs):
        if callback_on_step_end_tensor_inputs is not None and not all(
                k in ("latents", "prompt_embeds", "negative_prompt_embeds") for k in callback_on_step_end_tensor_inputs):
            raise ValueError(f"`callback_on_step_end_tensor_inputs` has to be in ['latents', 'prompt_embeds', "
                             f"'negative_prompt_embeds'], but found {callback_on_step_end_tensor_inputs}")
        if prompt is not None and prompt_embeds is not None:
            raise ValueError(f"Cannot forward both `prompt`: {prompt} and `prompt_embeds`: {prompt_embeds}. Please make sure to"
                             " only forward one of the two.")
        if prompt is None and prompt_embeds is None:
            raise ValueError("Provide either `prompt` or `prompt_embeds`. Cannot leave both `prompt` and `prompt_embeds` undefined.")
        if prompt is not None and (self.text_encoder is None or self.text_encoder_2 is None or self.tokenizer is None):
            raise NotImplementedError("`prompt` strings need text encoders + tokenizers attached to the pipeline "
                                      "(tokenizer vocabularies are not available offline): pass `prompt_embeds` / "
                                      "`pooled_prompt_embeds`, or `prompt_ids` / `prompt_ids_2`")
        if prompt_embeds is not None and negative_prompt_embeds is not None and prompt_embeds.shape != negative_prompt_embeds.shape:
            raise ValueError("`prompt_embeds` and `negative_prompt_embeds` must have the same shape when passed directly, but"
                             f" got: `prompt_embeds` {prompt_embeds.shape} != `negative_prompt_embeds` {negative_prompt_embeds.shape}.")
        if prompt is None and prompt_embeds is not None and pooled_prompt_embeds is None:
            raise ValueError("If `prompt_embeds` are provided, `pooled_prompt_embeds` also have to be passed. Make sure to "
                             "generate `pooled_prompt_embeds` from the same text encoder that was used to generate `prompt_embeds`.")
        if negative_prompt_embeds is not None and negative_pooled_prompt_embeds is None:
            raise ValueError("If `negative_prompt_embeds` are provided, `negative_pooled_prompt_embeds` also have to be passed.")
        s, e = control_guidance_start, control_guidance_end
        if s >= e:
            raise ValueError(f"control guidance start: {s} cannot be larger or equal to control guidance end: {e}.")
        if s < 0.0:
            raise ValueError(f"control guidance start: {s} can't be smaller than 0.")
        if e > 1.0:
            raise ValueError(f"control guidance end: {e} can't be larger than 1.0.")
        if ip_adapter_image is not None and ip_adapter_image_embeds is not None:
            raise ValueError("Provide either `ip_adapter_image` or `ip_adapter_image_embeds`. Cannot leave both "
                             "`ip_adapter_image` and `ip_adapter_image_embeds` defined.")
        if ip_adapter_image_embeds is not None:
            if not isinstance(ip_adapter_image_embeds, list):
                raise ValueError(f"`ip_adapter_image_embeds` has to be of type `list` but is {type(ip_adapter_image_embeds)}")
            if ip_adapter_image_embeds[0].ndim not in [3, 4]:
                raise ValueError("`ip_adapter_image_embeds` has to be a list of 3D or 4D tensors but is "
                                 f"{ip_adapter_image_embeds[0].ndim}D")

    def encode_prompt(self, prompt=None, prompt_2=None, negative_prompt=None, negative_prompt_2=None, prompt_ids=None,
                      prompt_ids_2=None, negative_prompt_ids=None, negative_prompt_ids_2=None, do_cfg=True, clip_skip=None):
        """`encode_prompt` (pipelines/sdxl_instantir.py:400-632) on the HIP text encoders: both CLIP encoders'
        hidden_states[-2] concatenated (B,77,2048) + the second encoder's projected EOS feature (B,1280).  Strings
        go through the attached tokenizers (77 tokens, padded / truncated); ids may be passed directly.  With no
        negative prompt the negative embeddings are zeros (`force_zeros_for_empty_prompt`, :567-571)."""
        from .encoders import encode_prompt_ids

        def ids_of(texts, tok):
            texts = [texts] if isinstance(texts, str) else list(texts)
            return tok(texts)

        if prompt_ids is None:
            prompt_ids = ids_of(prompt, self.tokenizer)
            prompt_ids_2 = ids_of(prompt_2 if prompt_2 is not None else prompt, self.tokenizer_2 or self.tokenizer)
        if prompt_ids_2 is None:
            prompt_ids_2 = prompt_ids
        def encode(ids, ids2, skip):
            # A batch job restores every image under the SAME prompt (infer.py:211-222): the two CLIP passes (~20 ms per prompt at
            # SDXL size) are kept per token-id pair -- the encoders are deterministic, the cached tensors are never written to.
            key = (ids.cpu().numpy().tobytes(), ids2.cpu().numpy().tobytes(), tuple(ids.shape), skip, id(self.text_encoder), id(self.text_encoder_2))
            hit = self._prompt_cache.get(key)
            if hit is None or hit[2] is not self.text_encoder or hit[3] is not self.text_encoder_2:
                hit = (*encode_prompt_ids(self.text_encoder, self.text_encoder_2, ids, ids2, skip), self.text_encoder, self.text_encoder_2)
                if len(self._prompt_cache) >= 8:
                    self._prompt_cache.pop(next(iter(self._prompt_cache)))
                self._prompt_cache[key] = hit
            return hit[0], hit[1]

        pe, pooled = encode(prompt_ids, prompt_ids_2, clip_skip)
        npe = npooled = None
        if do_cfg:
            if negative_prompt_ids is None and negative_prompt is not None:
                negative_prompt_ids = ids_of(negative_prompt, self.tokenizer)
                negative_prompt_ids_2 = ids_of(negative_prompt_2 if negative_prompt_2 is not None else negative_prompt,
                                               self.tokenizer_2 or self.tokenizer)
            if negative_prompt_ids is None:
                npe, npooled = torch.zeros_like(pe), torch.zeros_like(pooled)
            else:
                # (the reference always takes hidden_states[-2] for the negative prompt, :586: clip_skip is not applied)
                npe, npooled = encode(negative_prompt_ids, negative_prompt_ids_2 if negative_prompt_ids_2 is not None else negative_prompt_ids, None)
        return pe, npe, pooled, npooled

    def encode_image(self, image):
        """`encode_image` (pipelines/sdxl_instantir.py:636-670): (features, zero-image features).  DINO branch (:660-667):
        `last_hidden_state`; CLIP branch as `prepare_ip_adapter_image_embeds` calls it for a Resampler projector (:696-699,
        :644-654): `hidden_states[-2]` of the image and of `zeros_like(image)`.
        `image`: PIL image(s) (pre-processed like the encoder's own image processor) or a normalised tensor."""
        from .encoders import HipCLIPVision, clip_preprocess, dinov2_preprocess
        if self.image_encoder is None:
            raise NotImplementedError("pass `ip_adapter_image_embeds` or attach an image encoder (encoders.HipDinov2)")
        pre = clip_preprocess if isinstance(self.image_encoder, HipCLIPVision) else dinov2_preprocess
        px = image if torch.is_tensor(image) else pre(image, device=self.device if self._device_preprocess else None)
        return self.image_encoder.encode_image_pair(px)

    def enable_device_preprocess(self):
        """`encode_image` preprocesses PIL images on the device (one uint8 upload, ops.resample with the crop as its window and
        the normalisation as its affine) instead of PIL on the host; at most 1 LSB from it before normalisation.  Off by default."""
        self._device_preprocess = True

    def disable_device_preprocess(self):
        self._device_preprocess = False

    # ---- device-side resize around the call (an addition; DESIGN.md section 7 "Resampling") ------------------------
    @staticmethod
    def _check_resize(work_size, output_size, resample, output_type, image=None, multiple=8):
        """Checks of `work_size` / `output_size` / `resample` -> the two sizes as (H, W) int tuples (or None)."""
        from . import resample as RS
        if resample not in RS.FILTERS:
            raise ValueError(f"resample must be one of {RS.FILTERS}, got {resample!r}")
        if work_size is None and output_size is None:
            if resample != "bilinear":
                raise ValueError(f"resample={resample!r} needs work_size or output_size: nothing is resampled without them")
            return None, None
        if work_size is not None:
            work_size = RS.check_size(work_size, "work_size", multiple)
            if torch.is_tensor(image) and image.dim() == 4 and image.shape[1] == 4:
                raise ValueError("work_size resamples pixels: `image` is an LQ latent (B,4,h,w)")
        if output_size is not None:
            output_size = RS.check_size(output_size, "output_size")
            if output_type == "latent":
                raise ValueError("output_size resamples decoded pixels: output_type='latent' leaves none to resample")
        return work_size, output_size

    def _resample_input(self, image, work_size, resample):
        """A pixel `image` of any size (PIL, numpy or a [0,1] tensor) at `work_size`, fp32 (n,3,H,W) in [0,1] on the device.
        8-bit inputs use quantised mode (PIL's semantics for such an image), float inputs float mode with a clamp to [0,1]."""
        from . import resample as RS
        if not torch.is_tensor(image) and not hasattr(image, "ndim"):
            image = [im.convert("RGB") if hasattr(im, "convert") else im for im in (image if isinstance(image, (list, tuple)) else [image])]
        batch, kind = RS.as_batch(image)
        if batch.shape[-1 if kind == "u8" else 1] != 3:
            raise ValueError(f"work_size takes RGB pixels, got {tuple(batch.shape)}")
        if kind == "u8":
            return RS.resize_images(batch, work_size, resample, self.device, quantize=True, scale=1.0 / 255.0)
        if batch.min() < 0:
            raise ValueError("work_size takes a float `image` in [0, 1]; this one has negative values (already normalised?)")
        return RS.resize_images(batch, work_size, resample, self.device, quantize=False, clamp=(0.0, 1.0))

    def _preprocess_work_image(self, image):
        """The working image (fp32 (n,3,H,W) in [0,1] on the device) as the image encoder's input: rounded to 8 bits -- the raw
        image a PIL copy of it would be -- and preprocessed on the device; `encode_image` takes the result as it stands."""
        from .encoders import HipCLIPVision, clip_preprocess, dinov2_preprocess
        pre = clip_preprocess if isinstance(self.image_encoder, HipCLIPVision) else dinov2_preprocess
        return pre((image * 255).round(), device=self.device)

    def _resample_output(self, img, output_size, resample, output_type):
        """The final [0,1] images (fp32 (B,3,H,W) on the device) at `output_size`, in the form `output_type` asks for.  'pil':
        rounded to 8 bits as `vae.to_output` rounds, then resampled in quantised mode, so the result is comparable with PIL's
        resize of the plain call's PIL output; 'np' / 'pt': float mode with a clamp to [0,1]."""
        if output_type == "pil":
            from PIL import Image
            out8 = ops.resample((img * 255).round(), output_size, resample, quantize=True)
            return [Image.fromarray(a) for a in out8.permute(0, 2, 3, 1).to(torch.uint8).cpu().numpy()]
        return self.vae.to_output(ops.resample(img.contiguous(), output_size, resample, clamp=(0.0, 1.0)), output_type)

    def prepare_ip_adapter_image_embeds(self, ip_adapter_image, do_cfg, batch=None):
        """:672-707 for one IP adapter: [(2 n, Bimg, S, E)] = cat([zero-image features, image features]) under CFG, each stacked
        n = `batch` // Bimg times (:1350-1357: torch.stack([e] * (B // e.shape[0]), dim=0); once without `batch`)."""
        f, z = self.encode_image(ip_adapter_image)                                 # (Bimg, S, E) features, zero-image features
        reps = max((batch or 0) // f.shape[0], 1)
        f, z = torch.stack([f] * reps, 0), torch.stack([z] * reps, 0)
        return [torch.cat([z, f]) if do_cfg else f]

    @staticmethod
    def _prepare_image(image):
        """`prepare_image` (:905-929) via VaeImageProcessor(do_normalize=True): PIL / numpy / [0,1] tensors
        become fp32 NCHW in [-1,1]; 4-channel tensors (latents) and tensors already below 0 pass through."""
        if torch.is_tensor(image):
            if image.shape[1] == 4 or image.min() < 0:
                return image
            return image * 2.0 - 1.0
        x = _image_array(image)
        if x.shape[2] % 8 or x.shape[3] % 8:
            raise ValueError(f"image size {tuple(x.shape[2:])} must be a multiple of 8 (infer.py:31-66 resizes to multiples of 64)")
        return x * 2.0 - 1.0

    # ---- LQ-guided colour fix of the final images (an addition; DESIGN.md section 7 "Colour fix") -----------------
    @staticmethod
    def _check_color_fix(color_fix, output_type):
        if color_fix not in COLOR_FIX_MODES:
            raise ValueError(f"color_fix must be None, 'wavelet' or 'adain', got {color_fix!r}")
        if color_fix is not None and output_type == "latent":
            raise ValueError("color_fix corrects decoded pixels: output_type='latent' leaves none to fix")

    def _color_fix_reference(self, color_fix_reference, image, B, nipp):
        """The colour reference of a call as fp32 (B,3,H,W) in [0,1] on the device.  `image` is what `_prepare_image` returned
        (before the VAE encode): pixels in [-1,1] serve as the default reference, an LQ latent cannot.  Expanded over the batch
        exactly as `lq` is (prepare_image :919-925)."""
        up = self.vae_scale_factor if image.shape[1] == 4 else 1
        height, width = image.shape[2] * up, image.shape[3] * up
        if color_fix_reference is None:
            if image.shape[1] == 4:
                raise ValueError("color_fix needs the LQ pixels: `image` is an LQ latent (B,4,h,w), so pass `color_fix_reference` "
                                 "(a [0,1] tensor or PIL image(s) of the output size)")
            ref = image.to(self.device, torch.float32) / 2 + 0.5
        elif torch.is_tensor(color_fix_reference):
            ref = color_fix_reference.to(self.device, torch.float32)
            if ref.dim() == 3:
                ref = ref.unsqueeze(0)
        else:
            ref = _image_array(color_fix_reference, same_size="color_fix_reference").to(self.device)
        if ref.dim() != 4 or ref.shape[1] != 3 or tuple(ref.shape[2:]) != (height, width):
            raise ValueError(f"color_fix reference has shape {tuple(ref.shape)}, expected (n, 3, {height}, {width}): the output's "
                             "size (no resampling is done here)")
        ref = ref.repeat(B, 1, 1, 1) if ref.shape[0] == 1 else ref.repeat_interleave(nipp, 0)
        if ref.shape[0] != B:
            raise ValueError(f"color_fix reference gives {ref.shape[0]} images, the batch has {B}")
        return ref.clamp(0, 1).contiguous()

    def _lq_latent(self, image, vae_noise):
        """The LQ latent, fp32 on the device, of what `_prepare_image` returned: a latent (B,4,h,w) as it stands, pixels through
        the VAE encoder (:1369-1379; `vae_noise`: the posterior sample's noise, drawn when None)."""
        if image.shape[1] != 4:
            if self.vae is None:
                raise NotImplementedError("pixel-space `image` needs a VAE; pass the LQ latent (B,4,h,w)")
            image = self.vae.encode_to_latent(image, eps=vae_noise)
        return image.to(self.device, torch.float32)

    def _decode_output(self, latents, output_type, color_fix=None, reference=None, composite=None, resize=None):
        """VAE decode of the final latents; with `color_fix` the decoded [0,1] image is corrected in place on the device
        (ops.colorfix) before it becomes 'np' / 'pil'; with `composite` = (original, pixel map, feather) of a restore map the
        kept region then gets the input's own pixels back (ops.region_composite, in place); with `resize` = (output size,
        filter) the result is then resampled on the device (`_resample_output`).  :1706-1729: any `output_type` but 'latent'
        needs the VAE."""
        if output_type == "latent":
            return latents
        if self.vae is None:
            raise NotImplementedError("output_type other than 'latent' needs a VAE attached to the pipeline")
        if color_fix is None and composite is None and resize is None:
            return self.vae.decode_latent(latents, output_type)          # tiles when `vae.enable_tiling()` is on
        img = self.vae.decode_latent(latents, "pt").contiguous()
        if color_fix is not None:
            ops.colorfix(img, reference, color_fix, out=img)
        if composite is not None:
            original, map_px, feather = composite
            ops.region_composite(img, original, map_px, feather, out=img)
        if resize is not None:
            return self._resample_output(img, resize[0], resize[1], output_type)
        return self.vae.to_output(img, output_type)

    # ---- single-step previewer restoration (BASELINE configs[4]; spec train_previewer_lora.py:118-145) ------------
    @torch.no_grad()
    def restore_single_step(self, image, prompt_embeds, pooled_prompt_embeds, ip_adapter_image_embeds=None,
                            ip_adapter_image=None, timestep: int = 999, previewer_scheduler=None, generator=None,
                            init_noise=None, output_type: str = "pil", fp8: bool = False, color_fix: Optional[str] = None,
                            color_fix_reference=None, **kwargs):
        """LCM one-step restoration with the previewer LoRA, no CFG (guidance 1.0): noise the LQ latent to `timestep`
        (`prepare_latents` there = scheduler.add_noise), ONE UNet pass with the LoRA enabled, `LCMSingleStepScheduler.step`
        (schedulers/lcm_single_step_scheduler.py:421-489), VAE decode.  `fp8=True` (BASELINE configs[4]): the transformer
        blocks' linear layers of that pass run on fp8-E4M3 weights (per-output-channel scales) AND fp8 activations, stored as
        such by the LayerNorm / attention / GEGLU launch that produces them (`ops.gemm_fp8`, `v_mfma_f32_16x16x32_fp8_fp8`; round 3) --
        a third weight set, built on first use; its tolerance is its own (45.8 dB against the fp32 oracle at SDXL shapes).
        `color_fix` / `color_fix_reference`: as for `__call__`."""
        self._check_color_fix(color_fix, output_type)
        if self._lora is None:
            raise RuntimeError("restore_single_step needs the previewer LoRA: call prepare_previewers(...)")
        if fp8:
            key8 = (self._active_adapter, 1.0, "fp8")            # one fp8 copy per adapter: `set_adapter` must not leave a stale one
            if key8 not in self._prev_nets:
                self._prev_nets[key8] = HipUNet(self.cfg, self._unet_sd, self.device, lora=self._lora, lora_scaling=self._lora_scaling,
                                                fp8_linear=True)
            net = self._unet_prev8 = self._prev_nets[key8]
        else:
            self._build()
            net = self._unet_prev
        self._apply_freeu(net)
        sched = previewer_scheduler if previewer_scheduler is not None else LCMSingleStepScheduler.from_config(self.scheduler.config)
        dev, cfg = self.device, self.cfg
        image = self._prepare_image(image)
        cf_ref = self._color_fix_reference(color_fix_reference, image, image.shape[0], 1) if color_fix is not None else None
        lq = self._lq_latent(image, kwargs.get("vae_noise")).contiguous()
        B, _, Hl, Wl = lq.shape
        if ip_adapter_image_embeds is None:
            ip_adapter_image_embeds = self.prepare_ip_adapter_image_embeds(ip_adapter_image, False)
        px = (Hl * self.vae_scale_factor, Wl * self.vae_scale_factor)
        time_ids = _time_ids([[px[0], px[1], 0, 0, px[0], px[1]]], B)
        st = net.prepare(prompt_embeds, pooled_prompt_embeds, time_ids, net.resampler(ip_adapter_image_embeds[0]), Hl, Wl)
        x, _ = self._initial_latents(sched, lq, timestep, generator, init_noise)
        lat16 = torch.zeros(B * Hl * Wl, CPAD, dtype=F16, device=dev)
        ops.pack_latent(x, lat16)
        t_dev = torch.full((B, 1), float(timestep), dtype=torch.float32, device=dev)
        eps = net.forward(lat16, t_dev, st)
        out16 = torch.zeros(B * Hl * Wl, CPAD, dtype=F16, device=dev)
        out = torch.empty(B, 4, Hl, Wl, dtype=torch.float32, device=dev)
        coef = torch.tensor(sched.preview_coefficients(timestep), dtype=torch.float32).to(dev)
        ops.lcm_step(eps, B, 1, coef, x, out16, out)
        return StableDiffusionXLPipelineOutput(images=self._decode_output(out, output_type, color_fix, cf_ref))

    # ---- the call: its stages, in the reference's order -----------------------------------------------------------
    def _check_call(self, color_fix, output_type, cross_attention_kwargs, pag_scale, pag_adaptive_scale, multistep_restore,
                    guidance_scale=None, guidance_rescale=0.0, seg_scale=None):
        """Checks of the arguments `check_inputs` does not see -> (LoRA scale, `pag_scale` with its default, whether PAG runs,
        `seg_scale` with its default, whether SEG runs)."""
        self._check_color_fix(color_fix, output_type)
        if self._apg is not None:
            if guidance_scale is not None and not guidance_scale > 1:
                raise ValueError(f"adaptive projected guidance (enable_apg) projects the classifier-free guidance update: "
                                 f"guidance_scale must be > 1, got {guidance_scale}; call pipe.disable_apg() to run without guidance")
            if guidance_rescale and float(guidance_rescale) > 0.0:
                raise ValueError(f"guidance_rescale={guidance_rescale} does not combine with adaptive projected guidance (enable_apg): "
                                 "the APG norm clamp (norm_threshold) addresses the same over-exposure; use one of the two")
        # :1531-1535 merges the caller's dict over {"temb": emb} and hands it to both UNet passes.  What a key can do there:
        # "scale" is popped by diffusers' UNet forward and scales every LoRA layer for that pass (it also sets the text-encoder
        # LoRA scale, :1324-1326 -- no text-encoder LoRA exists on this path); "temb" / "external_kv" are the processors' own
        # arguments (module/ip_adapter/attention_processor.py:1093-1100): the loop owns `temb`, and no caller passes `external_kv`;
        # any other key is a TypeError inside the reference's processors.  "scale" is honoured by building the previewer's
        # merged copy with scale * alpha / r; the rest is refused with the reason.
        lora_mult = 1.0
        if cross_attention_kwargs:
            extra = set(cross_attention_kwargs) - {"scale"}
            if extra:
                raise ValueError(f"cross_attention_kwargs keys {sorted(extra)} are not accepted: the TA-IP attention processors take "
                                 "`temb` (set by the loop) and nothing a caller may override; only 'scale' (LoRA scale) is honoured")
            lora_mult = float(cross_attention_kwargs["scale"])
        if self._pag_layers is None and (pag_scale is not None or pag_adaptive_scale):
            raise ValueError("pag_scale / pag_adaptive_scale need perturbed-attention guidance: call pipe.enable_pag(...) first")
        if self._pag_layers is not None:
            pag_scale = pag.DEFAULT_PAG_SCALE if pag_scale is None else float(pag_scale)
        pag_on = self._pag_layers is not None and pag_scale > 0
        if self._seg_layers is None and seg_scale is not None:
            raise ValueError("seg_scale needs smoothed-energy guidance: call pipe.enable_seg(...) first")
        if self._seg_layers is not None:
            seg_scale = seg.check_scale(seg.DEFAULT_SEG_SCALE if seg_scale is None else seg_scale)
        seg_on = self._seg_layers is not None and seg_scale > 0
        if multistep_restore:
            raise NotImplementedError("multistep_restore passes kwargs the shipped DDPM scheduler does not accept "
                                      "(SURVEY.md Appendix C Q5)")
        return lora_mult, pag_scale, pag_on, seg_scale, seg_on

    def _embedding_rows(self, prompt, prompt_2, negative_prompt, negative_prompt_2, ids, prompt_embeds, negative_prompt_embeds,
                        pooled_prompt_embeds, negative_pooled_prompt_embeds, do_cfg, clip_skip, nipp):
        """Prompt embeddings (:1325-1348; encoded unless given, `ids`: the call's extra keyword arguments), one row per image, as the
        UNet's context and pooled rows in CFG order [negative; positive] (:1456-1464); and the negative ones, for the callback."""
        if prompt_embeds is None:
            prompt_embeds, ne, pooled_prompt_embeds, npool = self.encode_prompt(
                prompt, prompt_2, negative_prompt, negative_prompt_2, ids.get("prompt_ids"), ids.get("prompt_ids_2"),
                ids.get("negative_prompt_ids"), ids.get("negative_prompt_ids_2"), do_cfg, clip_skip)
            if negative_prompt_embeds is None:
                negative_prompt_embeds, negative_pooled_prompt_embeds = ne, npool
        if nipp > 1:            # diffusers encode_prompt: embeds.repeat(1, n, 1).view(bs * n, ...) == repeat_interleave
            prompt_embeds, pooled_prompt_embeds, negative_prompt_embeds, negative_pooled_prompt_embeds = (
                None if v is None else v.repeat_interleave(nipp, 0)
                for v in (prompt_embeds, pooled_prompt_embeds, negative_prompt_embeds, negative_pooled_prompt_embeds))
        if not do_cfg:
            return prompt_embeds, pooled_prompt_embeds, negative_prompt_embeds
        if negative_prompt_embeds is None:
            negative_prompt_embeds = torch.zeros_like(prompt_embeds)               # force_zeros_for_empty_prompt
            negative_pooled_prompt_embeds = torch.zeros_like(pooled_prompt_embeds)
        return (torch.cat([negative_prompt_embeds, prompt_embeds], 0), torch.cat([negative_pooled_prompt_embeds, pooled_prompt_embeds], 0),
                negative_prompt_embeds)

    def _image_rows(self, ip_adapter_image, ip_adapter_image_embeds, do_cfg, pb, nipp):
        """The image-embedding rows handed to the Resampler, (n, B, S, E) with CFG order [zero image; image]."""
        B = pb * nipp
        if ip_adapter_image_embeds is None:
            img = self.prepare_ip_adapter_image_embeds(ip_adapter_image, do_cfg, B)[0]
        else:
            # :709-722: each CFG half ([negative; positive]) repeated per prompt copy
            img = torch.cat([h.repeat(nipp, *([1] * (h.dim() - 1))) for h in ip_adapter_image_embeds[0].chunk(2 if do_cfg else 1)])
        if img.dim() == 3:
            img = img.unsqueeze(0)
        n_rows, R = img.shape[0] * img.shape[1], (2 if do_cfg else 1) * B
        if n_rows != R:
            raise ValueError(f"image embeds give {n_rows} rows, the batch has {R} (prompts {pb} x images-per-prompt {nipp}"
                             f"{' x 2 (CFG)' if do_cfg else ''})")
        return img

    def _timetable(self, timesteps, num_inference_steps, denoising_end, control_guidance_start, control_guidance_end, preview_start,
                   preview_end, controlnet_conditioning_scale):
        """Timetable and per-step gates (:1385, :1415-1425) -> (timesteps, `controlnet_keep`, previewing gate, conditioning scales)."""
        sigma_form = _sched_form(self.scheduler) == "hist"
        if timesteps is not None and sigma_form:
            raise ValueError(f"timesteps= is not supported with {type(self.scheduler).__name__} (custom sigma timetables are out of "
                             "scope); pass num_inference_steps, or use DDPMScheduler / DDIMScheduler for a hand-built timetable")
        if timesteps is not None:                                                   # retrieve_timesteps, :195-237
            self.scheduler.set_timesteps(timesteps=list(timesteps), device=None)
        else:
            self.scheduler.set_timesteps(num_inference_steps, device=None)
        # sigma schedulers: the float timestep reaches the UNet and the Aggregator (Karras timetables are fractional)
        ts = [float(t) if sigma_form else int(t) for t in self.scheduler.timesteps]
        n = len(ts)
        gate = lambda start, end: [1.0 - float(i / n < start or (i + 1) / n > end) for i in range(n)]      # noqa: E731
        keep, previewing = gate(control_guidance_start, control_guidance_end), gate(preview_start, preview_end)
        ccs = controlnet_conditioning_scale if isinstance(controlnet_conditioning_scale, list) else [controlnet_conditioning_scale] * n
        assert len(ccs) == n, f"{len(ccs)} controlnet scales do not match number of sampling steps {n}"
        if denoising_end is not None and isinstance(denoising_end, float) and 0 < denoising_end < 1:      # :1470-1483
            cutoff = int(round(self.scheduler.config.num_train_timesteps - denoising_end * self.scheduler.config.num_train_timesteps))
            ts = [t for t in ts if t >= cutoff]
        return ts, keep, previewing, ccs

    def _initial_latents(self, sched, lq, t0, generator, init_noise, init_latents_with_lq=True, latents=None):
        """:1388-1403: the LQ latent noised to the first timestep `t0`, or `latents` / a draw scaled by `init_noise_sigma`
        -> (the latents, `noise0`: the unit-variance tensor that seeded them, which a restore map's kept pixels follow)."""
        dev = self.device
        if not init_latents_with_lq:
            latents = _randn(lq.shape, generator, dev) if latents is None else latents
            noise0 = latents.to(dev, torch.float32)
            return (noise0 * sched.init_noise_sigma).contiguous(), noise0
        init_noise = _randn(lq.shape, generator, dev) if init_noise is None else init_noise
        noise0 = init_noise.to(dev, torch.float32)
        return sched.add_noise(lq, noise0, torch.tensor([t0] * lq.shape[0])).contiguous(), noise0

    def _denoise(self, x, ctx, loop_of, ts, keep, previewing, ccs, lq, reference_latents, previewer_scheduler, guidance_scale, eta,
                 generator, step_noises, pag_scale, pag_adaptive_scale, adastep_restore, save_preview_row, callback_on_step_end,
                 callback_on_step_end_tensor_inputs, negative_prompt_embeds, masked=False):
        """The denoising loop (:1497-1660) on the latents `x` -> (final latents, preview latents of each previewing step).
        `loop_of(ctx, fresh)`: the hoisted states and the `_DenoiseLoop` of a context."""
        loop = loop_of(ctx, False)
        B, rep, groups, pag_on, dev = loop.B, loop.rep, loop.groups, loop.pag_on, self.device
        preview_row = []
        thr = rmap.thresholds(len(ts)) if masked else None
        preview_factor = torch.ones(B)
        compound = None            # per-image scale the Aggregator's (persistent, raw) outputs currently carry
        pv = None                  # positive half of `preview_latent`: what conditioned the Aggregator last (:1545-1582)
        if adastep_restore and rep == 1:
            raise ValueError("adastep_restore slices preview_latent[B:], which is empty without classifier-free guidance "
                             "(pipelines/sdxl_instantir.py:1638; SURVEY.md Appendix C Q6)")
        for i, t in enumerate(ts):
            have_previewer = loop.st_prev is not None and previewer_scheduler is not None
            scale_rows = torch.clamp(preview_factor, 0.0, ccs[i]) * keep[i]            # :1538-1540
            use_agg = bool((scale_rows > 0.1).sum().item() > 0)                      # :1542
            if use_agg:
                mode = "preview" if (previewing[i] > 0 and have_previewer) else "agg"
                if previewing[i] > 0 and not have_previewer:
                    raise RuntimeError("previewing requested but no previewer: call prepare_previewers(...) and pass "
                                       "previewer_scheduler=LCMSingleStepScheduler")
                compound = scale_rows.clone()
            elif compound is None:
                raise RuntimeError("control_guidance_start > 0 leaves no aggregator residuals for step 0 "
                                   "(the reference fails with NameError here, SURVEY.md Appendix C Q2)")
            else:
                # :1602-1603 run unconditionally: the PREVIOUS step's already scaled residuals are scaled again (Q2).
                # Zero everywhere (the creative phase, keep = 0) -> the adds are skipped, which is the same result.
                compound = compound * scale_rows
                mode = "unet_res" if bool((compound != 0).any()) else "unet"
            x0 = loop.step(mode, t, x, (compound if mode != "unet" else scale_rows).repeat(groups), guidance_scale, eta,
                           None if step_noises is None else step_noises[i], generator, want_x0=adastep_restore, want_preview=save_preview_row or adastep_restore, i=i,
                           pag_s=pag.scale_at(pag_scale, pag_adaptive_scale, t) if pag_on else 0.0,
                           keep_row=(thr[i],) + rmap.keep_pair(self.scheduler, i, t) if masked else None, apg=self._apg)
            if mode == "preview":
                pv = loop.preview_f32[B * (rep - 1):]
                if save_preview_row:
                    preview_row.append(pv.clone().cpu())
            elif mode == "agg":
                pv = reference_latents.to(dev, torch.float32) if reference_latents is not None else lq     # :1579-1582
            if adastep_restore:                                                    # :1636-1644
                pv = pv.float().clone()
                pred_x0_l2 = (pv - x0).pow(2).sum(dim=(1, 2, 3))
                prev_l2 = (pv - loop.previewer_mean).pow(2).sum(dim=(1, 2, 3))
                loop.previewer_mean = pv
                preview_factor = (pred_x0_l2 / prev_l2).cpu()
            if callback_on_step_end is not None:                                   # :1646-1659
                named = {"latents": x, "prompt_embeds": ctx, "negative_prompt_embeds": negative_prompt_embeds}      # (the CFG-concatenated context)
                cb_in = {"latents": x, **{k: named[k] for k in (callback_on_step_end_tensor_inputs or [])}}
                cb = callback_on_step_end(self, i, t, cb_in)
                x = cb.pop("latents", x)
                new_ctx = cb.pop("prompt_embeds", None)
                cb.pop("negative_prompt_embeds", None)       # the reference rebinds a name it never reads again (:1465, :1655): no effect
                if new_ctx is not None and new_ctx is not ctx:
                    # the text K / V^T of all 70 cross-attention blocks are hoisted per call: a replaced context means hoisting
                    # again (and a new captured step), after which the loop continues on the same latents
                    if tuple(new_ctx.shape) != tuple(ctx.shape):
                        raise ValueError(f"callback_on_step_end returned prompt_embeds of shape {tuple(new_ctx.shape)}, expected {tuple(ctx.shape)}")
                    ctx = new_ctx
                    mean_keep, hist_keep, apg_keep = loop.previewer_mean, loop.hist, (loop.apg_avg, loop.apg_first)
                    loop = loop_of(ctx, True)
                    loop.previewer_mean = mean_keep
                    if hist_keep is not None:                # a multistep solver's x0 history continues across the rebuild
                        loop.hist.copy_(hist_keep)
                    if apg_keep[0] is not None and loop.apg_avg is not None:      # and so does APG's running average
                        loop.apg_avg.copy_(apg_keep[0])
                        loop.apg_first = apg_keep[1]
        return x, preview_row

    @torch.no_grad()
    def __call__(self, prompt=None, prompt_2=None, image=None, height=None, width=None, num_inference_steps: int = 30,
                 timesteps: List[int] = None, denoising_end: Optional[float] = None, guidance_scale: float = 7.0,
                 negative_prompt=None, negative_prompt_2=None, num_images_per_prompt: Optional[int] = 1, eta: float = 0.0,
                 generator=None, latents=None, prompt_embeds=None, negative_prompt_embeds=None, pooled_prompt_embeds=None,
                 negative_pooled_prompt_embeds=None, ip_adapter_image=None, ip_adapter_image_embeds=None,
                 output_type: Optional[str] = "pil", return_dict: bool = True, save_preview_row: bool = False,
                 init_latents_with_lq: bool = True, multistep_restore: bool = False, adastep_restore: bool = False,
                 cross_attention_kwargs=None, guidance_rescale: float = 0.0, controlnet_conditioning_scale=1.0,
                 control_guidance_start: float = 0.0, control_guidance_end: float = 1.0, preview_start: float = 0.0,
                 preview_end: float = 1.0, original_size=None, crops_coords_top_left=(0, 0), target_size=None,
                 negative_original_size=None, negative_crops_coords_top_left=(0, 0), negative_target_size=None,
                 clip_skip=None, callback_on_step_end: Optional[Callable] = None,
                 callback_on_step_end_tensor_inputs: List[str] = ["latents"], previewer_scheduler=None,
                 reference_latents=None, init_noise=None, step_noises=None, pag_scale: Optional[float] = None,
                 pag_adaptive_scale: float = 0.0, color_fix: Optional[str] = None, color_fix_reference=None, restore_map=None,
                 map_feather: int = 4, seg_scale: Optional[float] = None, work_size=None, output_size=None,
                 resample: str = "bilinear", **kwargs):
        """Keyword arguments and defaults of pipelines/sdxl_instantir.py:1067-1115.  Two additions for
        bit-reproducible parity runs: `init_noise` (the randn of init_latents) and
        `step_noises` (list of per-step DDPM / Euler-ancestral / DPM++ SDE noises) replace draws from `generator` when given.
        With a sigma scheduler (Euler, Euler-ancestral, DPM++) `eta` is ignored, as diffusers drops it for those `step()`s.
        `image` must be the LQ *latent* (B,4,h,w) here unless a VAE is attached (`image.shape[1] == 4` branch of :1369-1382).
        `pag_scale` / `pag_adaptive_scale` (an addition, after diffusers' PAG pipelines): need `enable_pag`; `pag_scale` None
        means 3.0, and PAG runs when it is > 0 (s_t = max(pag_scale - pag_adaptive_scale * (1000 - t), 0) per step).
        `seg_scale` (an addition, smoothed-energy guidance): needs `enable_seg`; None means 3.0, SEG runs when it is > 0, and the
        scale is the same at every step.
        `color_fix` (an addition, after StableSR's colour fixes): None, "wavelet" or "adain" transfers the colour of the LQ image
        onto the final images (never the preview row) after the VAE decode.  The reference is the pixel `image` mapped to
        [0, 1] unless `color_fix_reference` (a [0, 1] tensor or PIL image(s) of the output size) is given.
        `restore_map` (an addition, after inpaint-style latent blending and its soft form, differential diffusion): a per-pixel
        strength in [0, 1] -- the fraction of the schedule, counted from its end, during which the pixel is denoised freely
        (1: every step, today's behaviour; 0: never, the pixel comes out as the LQ input; until then it follows the LQ latent's
        own noising trajectory).  A PIL image ("L", / 255) or a list of them, or a tensor / array (H, W) or (B|1, 1, H, W), at
        the pixel size of `image` or at latent size; one map serves the whole batch, otherwise maps repeat per
        `num_images_per_prompt` copy.  At latent resolution a pixel is free if any pixel of its 8 x 8 block is.  When `image` was
        given as pixels and `output_type` is not "latent", the final images (never the preview row) are composited with the
        input after the decode and `color_fix`: a box window of half width `map_feather` pixels (default 4; 0 = hard paste)
        over [map > 0] weights decoded against input, and a pixel whose window lies wholly in the kept region is the input
        pixel bit for bit.  None touches nothing.
        `work_size` / `output_size` / `resample` (an addition: the resizes of infer.py:31-66 and :224-225 on the device, with
        PIL's filter definitions; `resample` one of "bilinear", "bicubic", "lanczos").  `work_size` = (H, W), multiples of 8: a
        pixel `image` of any size (PIL, numpy or a [0, 1] tensor) is resampled to it before anything else looks at it -- the
        result is what the VAE encodes, the default colour-fix reference, the composite's original and the default
        `ip_adapter_image` (then preprocessed on the device); 8-bit inputs resample as PIL resamples an 8-bit image, float
        tensors in float mode with a clamp to [0, 1]; `restore_map` sizes refer to the working size.  `output_size` = (H, W):
        the final images (never the preview row) are resampled after the decode, `color_fix` and the composite; "pil" rounds
        to 8 bits first and resamples as PIL would, "np" / "pt" resample in float mode with a clamp to [0, 1].  With all
        three at their defaults nothing is resampled."""
        work_size, output_size = self._check_resize(work_size, output_size, resample, output_type, image, self.vae_scale_factor)
        if restore_map is not None:
            map_feather = rmap.check_feather(map_feather)
        lora_mult, pag_scale, pag_on, seg_scale, seg_on = self._check_call(
            color_fix, output_type, cross_attention_kwargs, pag_scale, pag_adaptive_scale, multistep_restore, guidance_scale,
            guidance_rescale, seg_scale)
        if seg_on:       # SEG rides PAG's row group, step forms and scalar slot: from here on it is "PAG" with a constant scale
            pag_on, pag_scale, pag_adaptive_scale = True, seg_scale, 0.0
        ids_given = prompt is None and prompt_embeds is None and kwargs.get("prompt_ids") is not None and self.text_encoder is not None
        prompt_embeds_chk = kwargs["prompt_ids"] if ids_given else prompt_embeds      # ids stand in for the prompt in the exclusivity checks
        self.check_inputs(prompt, prompt_embeds_chk, negative_prompt_embeds,
                          pooled_prompt_embeds if prompt_embeds_chk is prompt_embeds else torch.zeros(1), negative_pooled_prompt_embeds,
                          ip_adapter_image, ip_adapter_image_embeds, control_guidance_start, control_guidance_end,
                          callback_on_step_end_tensor_inputs)
        self._guidance_scale = guidance_scale
        do_cfg = self.do_classifier_free_guidance
        self._build(lora_mult)

        nipp = int(num_images_per_prompt or 1)
        rep = 2 if do_cfg else 1      # row groups of the previewer and the Aggregator; the main UNet: [uncond;] cond [; perturbed]
        ctx, pooled, negative_prompt_embeds = self._embedding_rows(
            prompt, prompt_2, negative_prompt, negative_prompt_2, kwargs, prompt_embeds, negative_prompt_embeds, pooled_prompt_embeds,
            negative_pooled_prompt_embeds, do_cfg, clip_skip, nipp)
        B = ctx.shape[0] // rep
        pb = B // nipp                                                             # `batch_size` of :1304-1315
        if work_size is not None:                                                  # before anything else looks at the image
            image = self._resample_input(image, work_size, resample)
        n_img = 1 if hasattr(image, "size") and not torch.is_tensor(image) and not isinstance(image, (list, tuple)) else len(image)
        assert pb == n_img or n_img == 1                                          # :1310-1315
        if ip_adapter_image is None and ip_adapter_image_embeds is None:           # :1278-1279 (see Q15 in the header)
            if torch.is_tensor(image) and image.dim() == 4 and image.shape[1] == 4:
                raise ValueError("`image` is an LQ latent (B,4,h,w): it cannot stand in for `ip_adapter_image` (the image encoder takes "
                                 "pixels); pass `ip_adapter_image` or `ip_adapter_image_embeds`")
            ip_adapter_image = image
            if work_size is not None and self.image_encoder is not None:
                ip_adapter_image = self._preprocess_work_image(image)

        # -- the LQ latent (:1369-1379)
        image = self._prepare_image(image)
        cf_ref = self._color_fix_reference(color_fix_reference, image, B, nipp) if color_fix is not None else None
        lq = self._lq_latent(image, kwargs.get("vae_noise"))
        # prepare_image :919-925: one image serves the whole batch, otherwise each image is repeated per prompt copy
        lq = (lq.repeat(B, 1, 1, 1) if lq.shape[0] == 1 else lq.repeat_interleave(nipp, 0)).contiguous()
        Hl, Wl = lq.shape[2], lq.shape[3]
        height, width = Hl * self.vae_scale_factor, Wl * self.vae_scale_factor

        keep_map = composite = None
        if restore_map is not None:
            pixels_in = image.shape[1] != 4
            will_composite = pixels_in and output_type != "latent"
            m, at_pixels = rmap.prepare(restore_map, B, nipp, (height, width), (Hl, Wl), self.device)
            if will_composite and not at_pixels:
                raise ValueError(f"restore_map is at latent size ({Hl}, {Wl}) but the call composites pixels (pixel `image`, "
                                 f"output_type={output_type!r}): pass the map at the image size ({height}, {width})")
            keep_map = ops.map_pool_max(m, self.vae_scale_factor) if at_pixels else m
            if will_composite:
                composite = (self._color_fix_reference(None, image, B, nipp), m, map_feather)

        self._unet.set_pag(self._pag_paths if pag_on and not seg_on else None, rep * B)          # (refuses an fp8 engine)
        self._unet.set_seg(self._seg_paths if seg_on else None, rep * B, self._seg_sigma, Hl, Wl)  # (and a grid beyond the blur's limit)
        ids = list(original_size or (height, width)) + list(crops_coords_top_left) + list(target_size or (height, width))     # :965-981
        neg_ids = ids
        if negative_original_size is not None and negative_target_size is not None:   # :1445-1454
            neg_ids = list(negative_original_size) + list(negative_crops_coords_top_left) + list(negative_target_size)
        if self.cfg.addition_time_embed_dim * len(ids) + self.cfg.pooled_dim != self.cfg.add_embed_in:
            raise ValueError(f"Model expects an added time embedding vector of length {self.cfg.add_embed_in}, but a vector of "
                             f"{self.cfg.addition_time_embed_dim * len(ids) + self.cfg.pooled_dim} was created.")
        # :1459,:1464 verbatim: cat([neg, pos]) then .repeat(B, 1) -- for B > 1 the rows alternate neg, pos, neg, ... while
        # the prompt rows are [neg x B; pos x B]; only observable when negative sizes differ from the positive ones
        time_ids = _time_ids([neg_ids, ids] if do_cfg else [ids], B)
        img = self._image_rows(ip_adapter_image, ip_adapter_image_embeds, do_cfg, pb, nipp)

        ts, keep, previewing, ccs = self._timetable(timesteps, num_inference_steps, denoising_end, control_guidance_start,
                                                    control_guidance_end, preview_start, preview_end, controlnet_conditioning_scale)

        # -- step-invariant device state: the Aggregator's here, the UNets' per context
        st_agg = self._agg.prepare(pooled, time_ids, Hl, Wl, out_rows=(rep + 1) * B if pag_on else None)

        keep_box = []              # (latent map, noise0) once the initial latents exist: the loop is built after them

        def loop_of(ctx_, fresh):
            st = self._main_state(ctx_, pooled, time_ids, img, Hl, Wl, B, rep, pag_on)
            prev = self._unet_prev
            st_prev = None if prev is None else prev.prepare(ctx_, pooled, time_ids, prev.resampler(img), Hl, Wl)
            return self._loop_for(B, rep, Hl, Wl, st, st_prev, st_agg, lq, reference_latents, previewer_scheduler, guidance_rescale,
                                  pag_on, fresh=fresh, keep=keep_box[0] if keep_box else None, apg_on=self._apg is not None,
                                  seg_on=seg_on)

        x, noise0 = self._initial_latents(self.scheduler, lq, ts[0], generator, init_noise, init_latents_with_lq, latents)
        if keep_map is not None:
            keep_box.append((keep_map, noise0))
        x, preview_row = self._denoise(x, ctx, loop_of, ts, keep, previewing, ccs, lq, reference_latents, previewer_scheduler,
                                       guidance_scale, eta, generator, step_noises, pag_scale, pag_adaptive_scale, adastep_restore,
                                       save_preview_row, callback_on_step_end, callback_on_step_end_tensor_inputs,
                                       negative_prompt_embeds, masked=keep_map is not None)
        image_out = self._decode_output(x, output_type, color_fix, cf_ref, composite,
                                        (output_size, resample) if output_size is not None else None)
        if save_preview_row and self.vae is not None and output_type != "latent":     # :1706-1729 (decoded independently, Q4)
            preview_row = [self.vae.decode_latent(pl, output_type) for pl in preview_row]
        if not return_dict:
            return (image_out, preview_row) if save_preview_row else (image_out,)
        return StableDiffusionXLPipelineOutput(images=image_out)


def _sched_form(scheduler):
    """"hist": a sigma scheduler (Euler, Euler-ancestral, DPM++) driven through `loop_coefficients`, c_in-scaled UNet input
    and iir_sched_step with IIR_STEP_HIST; "linear": DDPM / DDIM through `step_coefficients` and iir_sched_step."""
    return "hist" if hasattr(scheduler, "loop_coefficients") else "linear"


def _scalar_row(rows, masked=False, apg=False):
    """Layout of a loop's per-step scalar row when its main UNet runs `rows` rows: ({name: slice}, length) of
    [t x rows | lcm coef x4 | sched coef x8 | res scale x rows | c_in | PAG s_t], and for a loop with a restore map (`masked`)
    [| keep x4] = {thr, a, b, 0} behind them, and for a loop with adaptive projected guidance (`apg`) [| apg x4] =
    {eta, r, beta_t, 0} behind everything else.  `sched` is the (8,) coefficient vector the iir_sched_step and PAG kernels index
    themselves: guidance in [0], the history term k_h in [7]."""
    lay, off = {}, 0
    groups = (("t", rows), ("lcm", 4), ("sched", 8), ("res_scale", rows), ("c_in", 1), ("pag_s", 1))
    for name, n in groups + ((("keep", 4),) if masked else ()) + ((("apg", 4),) if apg else ()):
        lay[name] = slice(off, off + n)
        off += n
    return lay, off


def _copy_state(dst, src):
    """Refresh a `prepare()` state in place (same structure, shapes and dtypes) so that launch sequences captured on `dst`'s
    tensors see `src`'s values.  `ada_jobs` is a device table of pointers into `dst`'s own tensors and stays.  False = the
    two states differ in structure: the caller builds a new loop."""
    if dst is None or src is None:
        return dst is None and src is None
    if dst.keys() != src.keys():
        return False
    for k, v in src.items():
        d = dst[k]
        if k == "ada_jobs":
            continue
        if isinstance(v, dict):
            if not isinstance(d, dict) or not _copy_state(d, v):
                return False
        elif isinstance(v, torch.Tensor):
            if not isinstance(d, torch.Tensor) or d.shape != v.shape or d.dtype != v.dtype or d.device != v.device:
                return False
            d.copy_(v)
        elif d != v:
            return False
    return True


class _DenoiseLoop:
    """Device buffers + (optionally hipGraph-captured) launch sequences of one denoising step.
    Three phases exist (pipelines/sdxl_instantir.py:1542-1616): "preview" (UNet+LoRA -> LCM preview
    -> Aggregator -> UNet), "agg" (Aggregator on the LQ / reference latent -> UNet), "unet".
    Rows: the previewer and the Aggregator run `rep` groups of B rows ([uncond;] cond), the main UNet `groups` of them --
    one more with perturbed-attention guidance (`pag_on`), whose rows copy the cond rows' inputs and residuals."""

    def __init__(self, pipe, B, rep, H, W, st, st_prev, st_agg, lq, reference_latents, previewer_scheduler, guidance_rescale=0.0,
                 pag_on=False, keep=None, apg_on=False):
        dev = pipe.device
        self.guidance_rescale = float(guidance_rescale or 0.0)
        self.cfg_factor = torch.ones(B, dtype=torch.float32, device=dev)
        self.p, self.B, self.rep, self.H, self.W = pipe, B, rep, H, W
        self.pag_on = bool(pag_on)
        self.groups = rep + int(self.pag_on)
        self.st, self.st_prev, self.st_agg = st, st_prev, st_agg
        self.prev_sched = previewer_scheduler
        R, HW = B * rep, H * W
        Rm = B * self.groups                                               # main UNet rows
        self.lat16 = torch.zeros(Rm * HW, CPAD, dtype=F16, device=dev)
        self.lat_prev = self.lat16[:R * HW]                                # the previewer's rows of it
        self.prev16 = torch.zeros(R * HW, CPAD, dtype=F16, device=dev)
        self.lq16 = torch.zeros(R * HW, CPAD, dtype=F16, device=dev)
        self.ref16 = torch.zeros(R * HW, CPAD, dtype=F16, device=dev) if reference_latents is not None else None
        ops.pack_latent(lq, self.lq16, rep=rep)
        if self.ref16 is not None:
            ops.pack_latent(reference_latents.to(dev, torch.float32).contiguous(), self.ref16, rep=rep)
        self.x_in = torch.empty(B, 4, H, W, dtype=torch.float32, device=dev)
        self.x_out = torch.empty_like(self.x_in)
        self.x0 = torch.empty_like(self.x_in)
        self.noise = torch.zeros_like(self.x_in)
        self.preview_f32 = torch.zeros(R, 4, H, W, dtype=torch.float32, device=dev)
        self.previewer_mean = torch.zeros_like(self.x_in)
        self.form = _sched_form(pipe.scheduler)
        # the x0 history of a multistep solver, read and rewritten in place by every step's iir_sched_step (IIR_STEP_HIST)
        self.hist = torch.zeros_like(self.x_in) if self.form == "hist" else None
        # restore map: the latent map, the fp32 LQ latent and the loop's seed noise, persistent so that captured launches see
        # the next call's values (`adopt`); {thr, a, b, 0} travels in the step's scalar row
        self.masked = keep is not None
        self.keep_map = self.keep_src = self.keep_noise = None
        if self.masked:
            self.keep_map = torch.empty(B, HW, dtype=torch.float32, device=dev)
            self.keep_src, self.keep_noise = torch.empty_like(self.x_in), torch.empty_like(self.x_in)
            self._adopt_keep(keep, lq)
        # adaptive projected guidance: the running average A of the guidance update, read and rewritten in place by every
        # step's iir_apg_project (in-place state, like `hist`), {s, alpha} per image and the reduction's workspace;
        # {eta, r, beta_t, 0} travels in the step's scalar row, beta_t = 0 on a call's first main-UNet step
        self.apg_on = bool(apg_on)
        self.apg_avg = torch.zeros_like(self.x_in) if self.apg_on else None
        self.apg_sa = torch.zeros(2 * B, dtype=torch.float32, device=dev) if self.apg_on else None
        self.apg_ws = ops.apg_workspace(B, dev) if self.apg_on else None
        self.apg_first = True
        lay, n_sc = _scalar_row(Rm, self.masked, self.apg_on)    # per-step scalars
        # ring of pinned staging rows: a row is rewritten only after the H2D copy that read it has completed
        self.sc_ring = [torch.zeros(n_sc, dtype=torch.float32).pin_memory() for _ in range(8)]
        self.sc_events = [None] * 8
        self.sc_idx = 0
        self.sc_dev, self.sc_lay = torch.zeros(n_sc, dtype=torch.float32, device=dev), lay
        self.t_dev = self.sc_dev[lay["t"]].view(Rm, 1)
        self.lcm_coef, self.sched_coef, self.res_scale, self.c_in, self.pag_s = (
            self.sc_dev[lay[k]] for k in ("lcm", "sched", "res_scale", "c_in", "pag_s"))
        self.keep_coef = self.sc_dev[lay["keep"]] if self.masked else None
        self.apg_par = self.sc_dev[lay["apg"]] if self.apg_on else None
        self.t_agg = self.t_dev[:R]                                         # the previewer's and the Aggregator's rows
        self.seg_jobs = None
        if self.pag_on:
            # one launch per Aggregator pass gives the perturbed rows of every residual the cond rows' values
            c0, c1, n = (rep - 1) * B, rep * B, self.groups * B
            outs = list(pipe._agg._out) + [pipe._agg._out_mid]
            jobs = []
            for o in outs:
                hw = o.shape[0] // n
                jobs.append((o[c0 * hw:c1 * hw], o[c1 * hw:n * hw]))
            self.seg_jobs = ops.segment_job_table(jobs, dev)
        self.graphs = {}
        self.side = None

    def _adopt_keep(self, keep, lq):
        kmap, noise0 = keep
        self.keep_map.copy_(kmap.reshape(self.B, -1))
        self.keep_src.copy_(lq)
        self.keep_noise.copy_(noise0)

    def adopt(self, st, st_prev, st_agg, lq, reference_latents, previewer_scheduler, keep=None):
        """Re-use this loop -- its buffers and captured graphs -- for another call of the same geometry: the new call's hoisted
        state (and restore map, `keep`) is copied into the tensors the graphs were captured on.  False when the states do not
        line up."""
        if (self.ref16 is None) != (reference_latents is None) or self.masked != (keep is not None):
            return False
        if not (_copy_state(self.st, st) and _copy_state(self.st_prev, st_prev) and _copy_state(self.st_agg, st_agg)):
            return False
        self.prev_sched = previewer_scheduler
        ops.pack_latent(lq, self.lq16, rep=self.rep)
        if self.ref16 is not None:
            ops.pack_latent(reference_latents.to(self.x_in.device, torch.float32).contiguous(), self.ref16, rep=self.rep)
        self.previewer_mean = torch.zeros_like(self.x_in)
        self.cfg_factor.fill_(1.0)
        if self.hist is not None:
            self.hist.zero_()
        if self.apg_on:
            self.apg_avg.zero_()
        self.apg_first = True
        if self.masked:
            self._adopt_keep(keep, lq)
        return True

    def _on_side(self, fn):
        """Run `fn` on the side stream, between a fork event recorded on the current stream now and a join event recorded behind
        it: (what `fn` returned, the join event)."""
        if self.side is None:
            self.side = torch.cuda.Stream(device=self.x_in.device)
        fork, join = torch.cuda.Event(), torch.cuda.Event()
        fork.record(torch.cuda.current_stream())
        self.side.wait_event(fork)
        with torch.cuda.stream(self.side):
            out = fn()
            join.record(self.side)
        return out, join

    def _condition(self, mode, want_preview, defer_shallow):
        """Previewer forward + LCM step (or the LQ / reference latent), Aggregator forward, PAG segment copy -> the residuals."""
        p = self.p
        if mode == "preview":
            eps1 = p._unet_prev.forward(self.lat_prev, self.t_agg, self.st_prev)          # :1545-1554
            ops.lcm_step(eps1, self.B, self.rep, self.lcm_coef, self.x_in, self.prev16,
                         self.preview_f32 if want_preview else None)                     # :1555-1561
            cond = self.prev16
        else:
            cond = self.ref16 if self.ref16 is not None else self.lq16               # :1579-1582
        p._agg.defer_shallow = defer_shallow
        down, mid = p._agg.forward(self.lq16, cond, self.t_agg, self.st_agg)           # :1591-1599
        if self.pag_on:
            ops.copy_segments(*self.seg_jobs)
        return down, mid

    def _launch(self, mode, use_noise, want_x0, want_preview, masked=False):
        p = self.p
        # scale_model_input(cat([latents]*2), t), :1503-1504: c_in from the step's scalar row (1 for DDPM / DDIM: x * 1 is exact)
        ops.pack_latent(self.x_in, self.lat16, rep=self.groups, scale=self.c_in)
        if mode == "unet":
            eps = p._unet.forward(self.lat16, self.t_dev, self.st)
        elif mode == "unet_res":     # stale residuals of the last Aggregator pass, re-scaled (see __call__)
            eps = p._unet.forward(self.lat16, self.t_dev, self.st, p._agg._out, p._agg._out_mid, self.res_scale)
        elif p.overlap_streams:
            # The main UNet's encoder half does not depend on the previewer / Aggregator: run it on a side
            # stream so its (CU-underfilling) launches overlap theirs; join before the residual adds.
            enc, join = self._on_side(lambda: p._unet.encode(self.lat16, self.t_dev, self.st))
            # (PAG: the perturbed rows' residuals are copied once every head has run, so no head is deferred)
            defer = p.overlap_sft and not self.pag_on
            down, mid = self._condition(mode, want_preview, defer)
            torch.cuda.current_stream().wait_event(join)
            late = None
            if defer:
                # the SFT heads of the shallow skips (consumed by the last up blocks) run on the side stream beside the
                # decoder's first up block
                _, late = self._on_side(p._agg.late_heads)
            eps = p._unet.decode(enc, self.st, down, mid, self.res_scale, late_event=late)
        else:
            down, mid = self._condition(mode, want_preview, False)
            eps = p._unet.forward(self.lat16, self.t_dev, self.st, down, mid, self.res_scale)
        self._sched(eps, use_noise, want_x0, masked)

    def _sched(self, eps, use_noise, want_x0, masked=False):
        """CFG (+ rescale_noise_cfg when guidance_rescale > 0, :181-192) + scheduler step, :1619-1633; `masked`: the restore-map
        form of the step, which selects the kept pixels' values inside the same launch."""
        B, rep = self.B, self.rep
        ps = self.pag_s if self.pag_on else None          # PAG forms: + s_t * (c - p), s_t read from the step's scalar row
        fac = None
        if rep == 2 and self.guidance_rescale > 0.0:
            fac = ops.cfg_rescale_factor(eps, B, self.sched_coef, self.x_in, self.guidance_rescale, self.cfg_factor, pag_scale=ps)
        apg = None
        if self.apg_on:
            apg = (self.apg_avg, self.apg_sa, self.apg_par)
            ops.apg_project(eps, B, self.sched_coef, self.x_in, apg, self.apg_ws)
        ops.sched_step(eps, B, self.sched_coef, self.x_in, self.x_out, noise=self.noise if use_noise else None, cfg=rep == 2,
                       x0_out=self.x0 if want_x0 else None, eps_factor=fac, pag_scale=ps, hist=self.hist,
                       keep=(self.keep_map, self.keep_src, self.keep_noise, self.keep_coef) if masked else None, apg=apg)

    def step(self, mode, t, x, res_scale_rows, guidance, eta, noise, generator, want_x0=False, want_preview=False, i=None,
             pag_s=0.0, keep_row=None, apg=None):
        """`i`: the step's index in the scheduler's timetable (the sigma schedulers' coefficients are per index).  `res_scale_rows`:
        one scale per main-UNet row.  `pag_s`: the step's PAG scale s_t.  `keep_row`: (thr, a, b) of a restore map for this step (a loop
        built with one).  `apg`: (eta, norm_threshold, momentum) of adaptive projected guidance (a loop built with it)."""
        p, lay = self.p, self.sc_lay
        slot = self.sc_idx % len(self.sc_ring)
        self.sc_idx += 1
        if self.sc_events[slot] is not None:
            self.sc_events[slot].synchronize()
        sc = self.sc_ring[slot]
        sc[lay["t"]] = float(t)
        c_in, t_lcm = 1.0, t
        if self.form == "hist":
            # eta is not an argument of these schedulers' step() (diffusers drops it): ignored
            lc = p.scheduler.loop_coefficients(i)
            c_in, t_lcm, coef = lc["c_in"], lc["t_lcm"], list(lc["coef"])
        else:
            coef = p.scheduler.step_coefficients(t, eta=eta)
        sc[lay["c_in"]] = c_in
        if mode == "preview":
            # a sigma scheduler's LCM previewer gets the scaled input c_in * x (:1555-1561) and t.to(int64) (:1557): fold c_in into
            # its coefficients so that iir_lcm_step reads the unscaled latent (c_in = 1 otherwise: / 1 and * 1 are exact)
            sb, sa, c_out, c_skip = self.prev_sched.preview_coefficients(t_lcm)
            sc[lay["lcm"]] = torch.tensor([sb / c_in, sa / c_in, c_out, c_skip * c_in])
        coef[0] = float(guidance)
        sc[lay["sched"]] = torch.tensor(coef)
        sc[lay["res_scale"]] = res_scale_rows.float()
        sc[lay["pag_s"]] = float(pag_s)
        if self.masked:
            sc[lay["keep"]] = torch.tensor(list(keep_row) + [0.0])
        if self.apg_on:
            # beta_t = 0 on the call's first main-UNet step: the average starts from this step's update alone
            sc[lay["apg"]] = torch.tensor([apg[0], apg[1], 0.0 if self.apg_first else apg[2], 0.0])
            self.apg_first = False
        use_noise = coef[6] != 0.0
        if use_noise:
            noise = _randn(self.x_in.shape, generator, self.x_in.device) if noise is None else noise
            self.noise.copy_(noise.to(self.noise.device, torch.float32), non_blocking=True)
        self.sc_dev.copy_(sc, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.sc_events[slot] = ev
        self.x_in.copy_(x)
        key = (mode, use_noise, want_x0, want_preview, self.masked)
        if p.use_graphs:
            g = self.graphs.get(key)
            if g is None:
                hist = self.hist.clone() if self.hist is not None else None
                avg = self.apg_avg.clone() if self.apg_on else None
                self._launch(*key)                        # warm-up: one-time attribute / workspace setup
                if hist is not None:
                    self.hist.copy_(hist)                 # the warm-up consumed the history: the replay below is the step
                if avg is not None:
                    self.apg_avg.copy_(avg)               # and overwrote APG's running average
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    self._launch(*key)
                self.graphs[key] = g
            g.replay()
        else:
            self._launch(*key)
        x.copy_(self.x_out)
        return self.x0 if want_x0 else None
