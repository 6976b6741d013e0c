"""GPU parity of the whole denoising loop (InstantIRPipeline over HIP) against the CPU oracle loop,
tiny geometry, identical seeded weights / inputs / noises.  Tolerance: latent PSNR (BASELINE.json
north_star asks >= 50 dB vs the reference latents at fp16)."""
import pytest
import torch

import loop_ref as lr
from loop_ref import dev, env  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


BAR = 50.0     # BASELINE.json north_star: latent PSNR >= 50 dB against the reference path at fp16


psnr = lr.psnr_by_caller("pipeline")


@pytest.mark.parametrize("graphs", [False, True])
def test_ddim_cfg_loop(env, graphs):
    from instantir_amd.schedulers import DDIMScheduler
    cfg, sd, sda, lora, inp = env
    want = lr.denoise(env, num_inference_steps=6, guidance_scale=7.0, sampler="ddim")
    pipe = lr.pipe(env, DDIMScheduler())
    pipe.use_graphs = graphs
    got = lr.call(pipe, inp, num_inference_steps=6, guidance_scale=7.0)
    p = psnr(got, want)
    assert torch.isfinite(got).all() and p >= BAR, p


def test_ddpm_phases_loop(env):
    """DDPM with explicit noises, preview_start / control_guidance_end gates: all three loop phases."""
    from instantir_amd.schedulers import DDPMScheduler
    cfg, sd, sda, lora, inp = env
    kw = dict(num_inference_steps=8, guidance_scale=5.0, preview_start=0.25, control_guidance_end=0.75)
    want = lr.denoise(env, sampler="ddpm", step_noises=inp["noises"], **kw)
    pipe = lr.pipe(env, DDPMScheduler())
    got = lr.call(pipe, inp, step_noises=inp["noises"], **kw)
    p = psnr(got, want)
    assert torch.isfinite(got).all() and p >= BAR, p


def test_guidance_rescale_loop(env):
    """guidance_rescale > 0: rescale_noise_cfg (pipelines/sdxl_instantir.py:181-192,1623-1626) inside the fused CFG + step."""
    from instantir_amd.schedulers import DDIMScheduler
    cfg, sd, sda, lora, inp = env
    kw = dict(num_inference_steps=4, guidance_scale=7.0, guidance_rescale=0.7)
    want = lr.denoise(env, sampler="ddim", **kw)
    plain = lr.denoise(env, sampler="ddim", num_inference_steps=4, guidance_scale=7.0)
    pipe = lr.pipe(env, DDIMScheduler())
    got = lr.call(pipe, inp, **kw)
    p = psnr(got, want)
    assert torch.isfinite(got).all() and p >= BAR, p
    assert psnr(got, plain) < p - 6          # the rescale is live: clearly closer to the rescaled oracle than to the plain one


def test_negative_size_conditioning(env):
    """negative_original_size / negative_target_size (pipelines/sdxl_instantir.py:1445-1464) reach the uncond rows' time ids."""
    from instantir_amd.schedulers import DDIMScheduler
    cfg, sd, sda, lora, inp = env
    kw = dict(num_inference_steps=2, guidance_scale=5.0)
    neg = (64, 96, 8, 4, 32, 48)
    want = lr.denoise(env, sampler="ddim", negative_time_ids=neg, **kw)
    plain = lr.denoise(env, sampler="ddim", **kw)
    pipe = lr.pipe(env, DDIMScheduler())
    got = lr.call(pipe, inp, negative_original_size=neg[:2], negative_crops_coords_top_left=neg[2:4], negative_target_size=neg[4:], **kw)
    p = psnr(got, want)
    assert p >= BAR and psnr(got, plain) < p - 6, (p, psnr(got, plain))


def test_aggregator_from_unet_emits_zero_residuals(env):
    """No aggregator weights loaded: the pipeline builds Aggregator.from_unet (module/aggregator.py:503-578) -- UNet encoder
    weights, SFT heads behind zero convolutions -- so every residual is zero; checked against the oracle given that state dict."""
    from instantir_amd.pipeline import InstantIRPipeline
    from instantir_amd.schedulers import DDIMScheduler
    cfg, sd, sda, lora, inp = env
    bare = InstantIRPipeline(cfg, sd, scheduler=DDIMScheduler())
    bare.prepare_previewers(lora, lora_alpha=16)
    agg = bare.aggregator.from_unet()
    assert set(agg) == set(sda) and all(agg[k].abs().max().item() == 0 for k in agg if k.startswith("controlnet_"))
    assert torch.equal(agg["ref_conv_in.weight"], sd["conv_in.weight"]) and torch.equal(agg["mid_block.resnets.0.conv1.weight"], sd["mid_block.resnets.0.conv1.weight"])
    got = lr.call(bare, inp, num_inference_steps=2, guidance_scale=5.0)
    want = lr.denoise((cfg, sd, agg, lora, inp), num_inference_steps=2, guidance_scale=5.0, sampler="ddim")
    trained = lr.denoise(env, num_inference_steps=2, guidance_scale=5.0, sampler="ddim")
    p = psnr(got, want)
    assert torch.isfinite(got).all() and p >= BAR and psnr(got, trained) < p - 6


def test_no_cfg_single_image(env):
    """BASELINE config 1 shape of the control flow: cfg = 1.0 (no CFG doubling), 4 steps."""
    from instantir_amd.schedulers import DDIMScheduler
    cfg, sd, sda, lora, inp = env
    one = {k: (v[:1] if torch.is_tensor(v) and v.shape[0] == inp["B"] else v) for k, v in inp.items()}
    one["img"] = inp["img"][1:, :1]
    one["B"] = 1
    from oracle import pipeline as OP
    P, PA, L = lr.params(env)
    want = OP.denoise(P, PA, L, cfg, one["lq"], one["pe"], one["pooled"], one["img"], init_noise=one["init_noise"],
                      num_inference_steps=4, guidance_scale=1.0, sampler="ddim")
    pipe = lr.pipe(env, DDIMScheduler())
    from instantir_amd.schedulers import LCMSingleStepScheduler
    got = pipe(image=one["lq"], prompt_embeds=one["pe"], pooled_prompt_embeds=one["pooled"],
               ip_adapter_image_embeds=[one["img"]], output_type="latent", num_inference_steps=4, guidance_scale=1.0,
               previewer_scheduler=LCMSingleStepScheduler.from_config(pipe.scheduler.config),
               init_noise=one["init_noise"]).images.float().cpu()
    p = psnr(got, want)
    assert p >= BAR, p


def test_single_step_previewer_restoration(env):
    """BASELINE configs[4] control flow: LQ latent noised to t = 999, one LoRA-UNet pass, LCM one-step x0, no CFG
    (train_previewer_lora.py:118-145; schedulers/lcm_single_step_scheduler.py:421-489)."""
    from instantir_amd.schedulers import DDPMScheduler
    from oracle import nets, sched
    cfg, sd, sda, lora, inp = env
    pipe = lr.pipe(env, DDPMScheduler())
    feats = inp["img"][1:]
    got = pipe.restore_single_step(inp["lq"], inp["pe"], inp["pooled"], ip_adapter_image_embeds=[feats], init_noise=inp["init_noise"],
                                   output_type="latent").images.float().cpu()
    P, _, L = lr.params(env)
    acp = sched.make_alphas_cumprod()
    B = inp["B"]
    x = sched.add_noise(acp, inp["lq"], inp["init_noise"], [999] * B)
    tid = torch.tensor([[128.0, 128, 0, 0, 128, 128]]).repeat(B, 1)
    ip = nets.image_projection(P, [feats], cfg.resampler, L)[0]
    eps = nets.unet_forward(P, cfg, x, 999, inp["pe"], inp["pooled"], tid, ip, lora=L)
    want = sched.lcm_step(acp, eps, 999, x)
    p = psnr(got, want)
    assert torch.isfinite(got).all() and p >= BAR, p


def test_adastep_restore_with_reference_latents_and_a_gated_step(env):
    """adastep_restore (pipelines/sdxl_instantir.py:1636-1644) with `reference_latents` (:1579-1580) and a per-step scale
    list whose third entry (0.05) puts every row below the 0.1 gate (:1542): that step skips previewer + Aggregator and
    re-scales the previous step's already scaled residuals (:1602-1603); the next step's factor is pred / 0 = inf,
    clamped back to the scale.  Checked against the oracle loop, which restates those statements one by one."""
    from instantir_amd.schedulers import DDIMScheduler
    cfg, sd, sda, lora, inp = env
    g = torch.Generator().manual_seed(7)
    ref = torch.randn(inp["B"], 4, inp["H"], inp["H"], generator=g) * 0.8
    kw = dict(num_inference_steps=5, guidance_scale=5.0, adastep_restore=True, reference_latents=ref, preview_end=0.4,
              controlnet_conditioning_scale=[1.0, 1.0, 0.05, 1.0, 1.0])
    trace = {}
    want = lr.denoise(env, sampler="ddim", trace=trace, **kw)
    modes = [bool((c > 0.1).any()) for c in trace["cond_scale"]]
    assert modes == [True, True, False, True, True]                         # the gated step is really exercised
    pipe = lr.pipe(env, DDIMScheduler())
    got = lr.call(pipe, inp, **kw)
    plain = lr.denoise(env, sampler="ddim", **{**kw, "adastep_restore": False})
    p = psnr(got, want)
    assert torch.isfinite(got).all() and p >= BAR and psnr(got, plain) < p - 6, (p, psnr(got, plain))


def test_adastep_needs_cfg(env):
    from instantir_amd.schedulers import DDIMScheduler
    cfg, sd, sda, lora, inp = env
    pipe = lr.pipe(env, DDIMScheduler())
    with pytest.raises(ValueError):
        lr.call(pipe, inp, num_inference_steps=2, guidance_scale=1.0, adastep_restore=True)


def test_denoising_end_custom_timesteps_and_callback(env):
    """`denoising_end` (:1470-1483) cuts the timetable while the gates keep the full step count; `timesteps=` (:195-237)
    hands the DDPM scheduler a custom descending list (previous timestep = next list entry); `callback_on_step_end`
    (:1651-1659) may replace the latents."""
    from instantir_amd.schedulers import DDIMScheduler, DDPMScheduler
    cfg, sd, sda, lora, inp = env
    kw = dict(num_inference_steps=6, guidance_scale=5.0, denoising_end=0.5)
    want = lr.denoise(env, sampler="ddim", **kw)
    pipe = lr.pipe(env, DDIMScheduler())
    seen = []

    def cb(p_, i, t, kwargs):
        seen.append((i, int(t)))
        return {"latents": kwargs["latents"]}

    got = lr.call(pipe, inp, callback_on_step_end=cb, **kw)
    assert seen == [(0, 831), (1, 665)]                  # N = 6 timetable 831, 665, 499, ...: cutoff 500 keeps two steps
    p = psnr(got, want)
    assert p >= BAR, p
    tlist = [901, 601, 301, 1]
    want = lr.denoise(env, sampler="ddpm", timesteps=tlist, guidance_scale=5.0, step_noises=inp["noises"])
    pipe2 = lr.pipe(env, DDPMScheduler())
    got = lr.call(pipe2, inp, timesteps=tlist, guidance_scale=5.0, step_noises=inp["noises"])
    p = psnr(got, want)
    assert p >= BAR, p


def test_callback_may_replace_prompt_embeds(env):
    """`callback_on_step_end` (:1646-1659) is handed the tensors it names and may hand back `prompt_embeds` (the CFG-concatenated
    context): unchanged -> bit-identical to a run without callback; replaced -> the text K / V of the cross-attention blocks are
    hoisted again and the remaining steps run on the new context (the result moves, stays finite); a wrong shape is refused."""
    from instantir_amd.schedulers import DDIMScheduler
    cfg, sd, sda, lora, inp = env
    pipe = lr.pipe(env, DDIMScheduler())
    kw = dict(num_inference_steps=4, guidance_scale=5.0)
    base = lr.call(pipe, inp, **kw)
    seen = []

    def same(p_, i, t, k):
        seen.append(tuple(k["prompt_embeds"].shape))
        return {"latents": k["latents"], "prompt_embeds": k["prompt_embeds"], "negative_prompt_embeds": k.get("negative_prompt_embeds")}

    got = lr.call(pipe, inp, callback_on_step_end=same, callback_on_step_end_tensor_inputs=["latents", "prompt_embeds", "negative_prompt_embeds"], **kw)
    assert torch.equal(got, base) and seen[0] == (2 * inp["B"], cfg.text_len, cfg.cross_attention_dim)

    def swap(p_, i, t, k):
        return {"prompt_embeds": (k["prompt_embeds"] * 0.25) if i == 1 else k["prompt_embeds"]}

    moved = lr.call(pipe, inp, callback_on_step_end=swap, callback_on_step_end_tensor_inputs=["prompt_embeds"], **kw)
    assert torch.isfinite(moved).all() and not torch.equal(moved, base)
    with pytest.raises(ValueError):
        lr.call(pipe, inp, callback_on_step_end=lambda p_, i, t, k: {"prompt_embeds": k["prompt_embeds"][:1]},
              callback_on_step_end_tensor_inputs=["prompt_embeds"], **kw)


def test_num_images_per_prompt(env):
    """num_images_per_prompt = 2 with ONE prompt / image: embeds repeat per prompt copy (diffusers encode_prompt), the LQ
    latent repeats over the batch (prepare_image :919-925), IP embeds repeat on dim 0 (:709-722).  Rows are independent, so
    each output row must equal the single-image run given the same noise row."""
    from instantir_amd.schedulers import DDIMScheduler
    cfg, sd, sda, lora, inp = env
    one = {k: (v[:1] if torch.is_tensor(v) and v.dim() > 0 and v.shape[0] == inp["B"] else v) for k, v in inp.items()}
    one["img"] = inp["img"][:, :1]
    pipe = lr.pipe(env, DDIMScheduler())
    noise2 = inp["init_noise"]                                             # (2,4,H,H): one row per generated image
    both = lr.call(pipe, {**one, "init_noise": noise2}, num_inference_steps=2, guidance_scale=5.0, num_images_per_prompt=2)
    assert both.shape[0] == 2
    for r in range(2):
        single = lr.call(pipe, {**one, "init_noise": noise2[r:r + 1]}, num_inference_steps=2, guidance_scale=5.0)
        # same kernels, same inputs: only what depends on the batch size differs -- tile shapes, and with them the grouping of
        # the LayerNorm partial statistics (per column tile of the producing GEMM); measured 61 dB over two steps
        assert psnr(both[r:r + 1], single) >= 55


def test_ip_adapter_image_defaults_to_image_and_preview_row(env):
    """`pipe(prompt_embeds=..., image=lq)` without ip_adapter_image (infer.py:211-222): it defaults to the LQ image
    (:1278-1279) and goes through `encode_image`; with no image encoder attached that is a clear error, with one attached
    the call runs.  `save_preview_row` (:1564-1567, :1706-1729) returns one preview per previewing step."""
    from instantir_amd.schedulers import DDIMScheduler, LCMSingleStepScheduler
    cfg, sd, sda, lora, inp = env
    pipe = lr.pipe(env, DDIMScheduler())
    lcm = LCMSingleStepScheduler.from_config(pipe.scheduler.config)
    base = dict(image=inp["lq"], prompt_embeds=inp["pe"], pooled_prompt_embeds=inp["pooled"], output_type="latent",
                negative_prompt_embeds=inp["npe"], negative_pooled_prompt_embeds=inp["npooled"], previewer_scheduler=lcm, init_noise=inp["init_noise"], num_inference_steps=3, guidance_scale=5.0)
    with pytest.raises(ValueError):                        # an LQ *latent* cannot stand in for the image encoder's input: said up front
        pipe(**base)

    class _Vae:                                            # pixel-space `image`: the VAE stand-in returns the fixture's LQ latent
        def encode_to_latent(self, image, eps=None, generator=None):
            assert image.shape[1] == 3 and image.min() >= -1.0 and image.max() <= 1.0
            return inp["lq"]

    pipe.vae = _Vae()
    base["image"] = torch.rand(inp["lq"].shape[0], 3, inp["lq"].shape[2] * 8, inp["lq"].shape[3] * 8, generator=torch.Generator().manual_seed(3))
    with pytest.raises(NotImplementedError):               # default ip_adapter_image = image, but no image encoder attached
        pipe(**base)

    class _Enc:                                            # stands in for encoders.HipDinov2: (features, zero-image features)
        def encode_image_pair(self, px):
            return inp["img"][1].to(px.device if torch.is_tensor(px) else "cpu"), inp["img"][0]

    pipe.image_encoder = _Enc()
    out, row = pipe(**base, return_dict=False, save_preview_row=True, preview_end=0.7)
    want = lr.call(pipe, inp, num_inference_steps=3, guidance_scale=5.0, preview_end=0.7)
    assert psnr(out.float().cpu(), want) >= 70
    assert len(row) == 2 and all(r.shape == inp["lq"].shape for r in row)     # steps 0 and 1 preview, step 2 does not


def test_single_step_previewer_restoration_fp8(env):
    """BASELINE configs[4]: the same single LCM step with the transformer linears on fp8-E4M3 weights.  Its tolerance is its
    own (8-bit operands with 3 mantissa bits; the reference has no fp8 path to compare with): asserted against the fp32
    oracle at >= 40 dB (measured 46.3) and against the fp16 HIP path at >= 40 dB; measured values go to gpurun_out/psnr.log."""
    from instantir_amd.schedulers import DDPMScheduler
    from oracle import nets, sched
    cfg, sd, sda, lora, inp = env
    pipe = lr.pipe(env, DDPMScheduler())
    feats = inp["img"][1:]
    kw = dict(ip_adapter_image_embeds=[feats], init_noise=inp["init_noise"], output_type="latent")
    got8 = pipe.restore_single_step(inp["lq"], inp["pe"], inp["pooled"], fp8=True, **kw).images.float().cpu()
    got16 = pipe.restore_single_step(inp["lq"], inp["pe"], inp["pooled"], **kw).images.float().cpu()
    P, _, L = lr.params(env)
    acp = sched.make_alphas_cumprod()
    B = inp["B"]
    x = sched.add_noise(acp, inp["lq"], inp["init_noise"], [999] * B)
    tid = torch.tensor([[128.0, 128, 0, 0, 128, 128]]).repeat(B, 1)
    ip = nets.image_projection(P, [feats], cfg.resampler, L)[0]
    want = sched.lcm_step(acp, nets.unet_forward(P, cfg, x, 999, inp["pe"], inp["pooled"], tid, ip, lora=L), 999, x)
    p_oracle, p_16 = psnr(got8, want), psnr(got8, got16)
    assert torch.isfinite(got8).all() and p_oracle >= 40 and p_16 >= 40, (p_oracle, p_16)
    assert not torch.equal(got8, got16)                      # the fp8 weight set is really in use


def test_adapter_switching_and_lora_scale(env):
    """Two LoRA adapters as in gradio_demo/app.py:67-69,114-120: `prepare_previewers(...)` registers `previewer`,
    `prepare_previewers(..., use_lcm=True)` registers `lcm` and -- like diffusers' `add_adapter` -- leaves the newest active;
    `pipe.unet.set_adapter` picks the one the previewer pass uses.  `cross_attention_kwargs={"scale": s}` (:1531-1535, popped by
    diffusers' UNet forward into `scale_lora_layers`) scales the active LoRA for that pass.  Each variant against the oracle
    loop run with that LoRA / scaling.  (peft / diffusers are absent here: their adapter bookkeeping is restated, unpinned.)"""
    from instantir_amd import weights as W
    from instantir_amd.schedulers import DDIMScheduler
    cfg, sd, sda, lora, inp = env
    lcm_lora = W.synth_state_dict(W.lora_specs(cfg, W.LCM_LORA_MODULES), 14)
    pipe = lr.pipe(env, DDIMScheduler())
    assert pipe.unet.active_adapters() == ["previewer"]
    assert pipe.prepare_previewers(lcm_lora, use_lcm=True, lora_alpha=8) == 8
    assert pipe.unet.active_adapters() == ["lcm"]
    kw = dict(num_inference_steps=2, guidance_scale=5.0)

    def oracle(lo, scaling):
        from oracle import pipeline as OP
        L = {k: v.float() for k, v in lo.items()}
        L["scaling"] = scaling
        return OP.denoise({k: v.float() for k, v in sd.items()}, {k: v.float() for k, v in sda.items()}, L, cfg, inp["lq"],
                          inp["pe"], inp["pooled"], inp["img"], negative_prompt_embeds=inp["npe"], negative_pooled=inp["npooled"],
                          init_noise=inp["init_noise"], sampler="ddim", **kw)

    got_lcm = lr.call(pipe, inp, **kw)
    assert psnr(got_lcm, oracle(lcm_lora, 8.0 / cfg.lora_rank)) >= BAR
    pipe.unet.set_adapter("previewer")
    got_prev = lr.call(pipe, inp, **kw)
    want_prev = oracle(lora, 16.0 / cfg.lora_rank)
    assert psnr(got_prev, want_prev) >= BAR
    assert psnr(got_lcm, want_prev) < BAR - 10                   # the two adapters really differ
    got_half = lr.call(pipe, inp, cross_attention_kwargs={"scale": 0.5}, **kw)
    assert psnr(got_half, oracle(lora, 0.5 * 16.0 / cfg.lora_rank)) >= BAR
    assert psnr(lr.call(pipe, inp, **kw), want_prev) >= BAR         # the unscaled copy is still the default afterwards
    with pytest.raises(ValueError):
        lr.call(pipe, inp, cross_attention_kwargs={"external_kv": None}, **kw)
    with pytest.raises(ValueError):
        pipe.unet.set_adapter("nope")

    # Replacing or releasing an engine drops the cached loop (its entry pins the engines it was captured on), and the next call
    # is bit-identical to a freshly built pipeline given the same adapters and inputs.
    def fresh(active):
        ref = lr.pipe(env, DDIMScheduler())
        ref.prepare_previewers(lcm_lora, use_lcm=True, lora_alpha=8)
        ref.unet.set_adapter(active)
        return lr.call(ref, inp, **kw3)

    kw3 = dict(num_inference_steps=3, guidance_scale=5.0)
    want = {name: fresh(name) for name in ("lcm", "previewer")}
    assert not torch.equal(want["lcm"], want["previewer"])
    lr.call(pipe, inp, **kw3)                                        # (`previewer` is active)
    assert pipe._loop_cache is not None
    pipe.unet.set_adapter("lcm")
    assert pipe._loop_cache is None
    assert torch.equal(lr.call(pipe, inp, **kw3), want["lcm"])
    assert pipe._loop_cache is not None
    pipe.prepare_previewers(lora, lora_alpha=16)                   # a second time: releases the merged `previewer` copies
    assert pipe._loop_cache is None and pipe.unet.active_adapters() == ["previewer"]
    assert torch.equal(lr.call(pipe, inp, **kw3), want["previewer"])
    assert pipe._loop_cache is not None
    pipe.aggregator.load_state_dict(sda)
    assert pipe._loop_cache is None
    assert torch.equal(lr.call(pipe, inp, **kw3), want["previewer"])


def test_step_graphs_are_reused_across_calls(env, monkeypatch):
    """A second image of the same geometry runs on the first call's buffers and captured graphs (its hoisted state is copied
    in): results must be bit-identical to calls that build everything afresh, in any order of inputs."""
    from instantir_amd.schedulers import DDIMScheduler
    cfg, sd, sda, lora, inp = env
    g = torch.Generator().manual_seed(77)
    inp_b = dict(inp)
    for k in ("lq", "pe", "pooled", "npe", "npooled", "img", "init_noise"):
        inp_b[k] = (torch.randn(inp[k].shape, generator=g) * 0.7).half().float()
    pipe = lr.pipe(env, DDIMScheduler())
    kw = dict(num_inference_steps=4, guidance_scale=7.0)
    a1 = lr.call(pipe, inp, **kw)
    loop = pipe._loop_cache[1]
    b1 = lr.call(pipe, inp_b, **kw)
    assert pipe._loop_cache[1] is loop, "second call of the same geometry built a new loop"
    a2 = lr.call(pipe, inp, **kw)
    assert pipe._loop_cache[1] is loop
    assert torch.equal(a1, a2) and not torch.equal(a1, b1)
    # a different number of rows (no classifier-free guidance): a new loop, and back again
    inp_c = dict(inp, img=inp["img"][1:])
    c1 = lr.call(pipe, inp_c, num_inference_steps=4, guidance_scale=1.0)
    assert pipe._loop_cache[1] is not loop
    a3 = lr.call(pipe, inp, **kw)
    assert torch.equal(a1, a3)
    monkeypatch.setenv("IIR_LOOP_CACHE", "0")
    fresh = lr.pipe(env, DDIMScheduler())
    assert torch.equal(lr.call(fresh, inp_b, **kw), b1)
    assert torch.equal(lr.call(fresh, inp_c, num_inference_steps=4, guidance_scale=1.0), c1)


def test_from_modules_matches_the_state_dict_constructor(env):
    """`InstantIRPipeline.from_modules(...)` -- the reference constructor's signature (pipelines/sdxl_instantir.py:303-322) fed with
    module objects (anything with `.state_dict()` / `.config`) -- builds the same pipeline as the state-dict constructor."""
    from instantir_amd.pipeline import InstantIRPipeline
    from instantir_amd.schedulers import DDIMScheduler
    cfg, sd, sda, lora, inp = env

    class Mod:                       # stand-in for a diffusers module: tensors + (optionally) a config object
        def __init__(self, tensors, **config):
            self._t = tensors
            if config:
                self.config = type("Config", (), config)()

        def state_dict(self):
            return self._t

    pipe = InstantIRPipeline.from_modules(unet=Mod(sd), aggregator=Mod(sda), scheduler=DDIMScheduler(), unet_config=cfg)
    pipe.prepare_previewers(lora, lora_alpha=16)
    ref = lr.pipe(env, DDIMScheduler())
    kw = dict(num_inference_steps=3, guidance_scale=7.0)
    assert torch.equal(lr.call(pipe, inp, **kw), lr.call(ref, inp, **kw))
    with pytest.raises(ValueError):
        InstantIRPipeline.from_modules(scheduler=DDIMScheduler())
