"""GPU: region-selective restoration (`restore_map=`; DESIGN.md section 7 "Restore map").

Kernel level: iir_sched_step_keep against the existing step entries and iir_axpby_f32 (bit equality on both sides of the
select), iir_map_pool_max_f32 against torch's max_pool2d, iir_region_composite_f32 against a restatement on integer counts.
Loop level: the fused map against the contract applied through `callback_on_step_end` (the mechanism a caller had before),
bit for bit, with hipGraph capture on; the two ends of the map; pixels in, pixels out; the cached loop; the CLI.
No tolerance anywhere: every comparison is on bits."""
import functools
import os

import numpy as np
import pytest
import torch

import loop_ref as lr
from loop_ref import dev  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

N_STEPS = 6


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


# ---- iir_sched_step_keep ------------------------------------------------------------------------------------------
B, C, H, W = 2, 4, 5, 7                                               # HW = 35: not a multiple of the block
HW = H * W
THR = float(np.float32(4 / 6))


def _map_values(shift):
    """0, exactly thr, the next float above thr, and 1, cycling over the pixels (another phase per image)."""
    vals = torch.tensor([0.0, THR, float(np.nextafter(np.float32(THR), np.float32(1.0))), 1.0], dtype=torch.float32)
    return vals[(torch.arange(HW) + shift) % 4]


def _step_case(dev, cfg, pag, hist, noise, fac, seed=0):
    g = torch.Generator().manual_seed(100 + seed)
    rows = B * ((2 if cfg else 1) + int(pag))
    t = dict(eps=torch.randn(rows * HW, 8, generator=g).half(), x=torch.randn(B, C, H, W, generator=g) * 3,
             coef=torch.tensor([6.5, 0.93, 0.37, 0.41, 0.98, 0.12, 0.07 if noise else 0.0, -0.031 if hist else 0.0]),
             lq=torch.randn(B, C, H, W, generator=g), noise0=torch.randn(B, C, H, W, generator=g),
             map=torch.stack([_map_values(0), _map_values(1)]))
    t["noise"] = torch.randn(B, C, H, W, generator=g) if noise else None
    t["hist"] = torch.randn(B, C, H, W, generator=g) if hist else None
    t["pag"] = torch.tensor([1.7]) if pag else None
    t["fac"] = torch.tensor([0.8, 1.3]) if fac else None
    return {k: None if v is None else v.to(dev) for k, v in t.items()}


def _run_step(t, cfg, keep_coef=None, want_eps=False):
    """One launch -> (prev, x0, hist after, eps_out): through iir_sched_step_keep with `keep_coef`, the matching existing entry
    without."""
    from instantir_amd import ops
    prev, x0 = torch.full_like(t["x"], 7.0), torch.full_like(t["x"], 7.0)
    hist = None if t["hist"] is None else t["hist"].clone()
    eps_out = torch.full_like(t["x"], 7.0) if want_eps else None
    keep = None if keep_coef is None else (t["map"], t["lq"], t["noise0"], keep_coef)
    ops.sched_step(t["eps"], B, t["coef"], t["x"], prev, noise=t["noise"], cfg=cfg, x0_out=x0, eps_out=eps_out, eps_factor=t["fac"],
                   pag_scale=t["pag"], hist=hist, keep=keep)
    torch.cuda.synchronize()
    return prev, x0, hist, eps_out


VARIANTS = {"plain": {}, "pag": dict(pag=True), "hist": dict(hist=True), "noise": dict(noise=True), "eps_factor": dict(fac=True),
            "all": dict(pag=True, hist=True, noise=True, fac=True)}


@pytest.mark.parametrize("cfg", [False, True], ids=["nocfg", "cfg"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_step_keep_selects_bits(dev, cfg, variant):
    from instantir_amd import ops
    v = dict(pag=False, hist=False, noise=False, fac=False)
    v.update(VARIANTS[variant])
    if not cfg:
        v["fac"] = False                                              # eps_factor belongs to the guided form
    t = _step_case(dev, cfg, **v)
    want_eps = not v["hist"]
    a, b = 0.62, 0.78
    kcoef = torch.tensor([THR, a, b, 0.0], device=dev)
    ref_prev, ref_x0, ref_hist, ref_eps = _run_step(t, cfg, want_eps=want_eps)
    prev, x0, hist, eps_out = _run_step(t, cfg, keep_coef=kcoef, want_eps=want_eps)
    kept = (t["map"] <= THR).reshape(B, 1, H, W).expand(B, C, H, W)
    # 0 and thr itself are kept, the next float above thr and 1 are free
    assert kept.reshape(B, C, HW)[0, 0, :4].tolist() == [True, True, False, False]
    keep_val = ops.axpby_f32(t["lq"], t["noise0"], torch.tensor([a, b], device=dev), torch.empty_like(t["lq"]))
    torch.cuda.synchronize()
    assert same_bits(prev[~kept], ref_prev[~kept])                    # a free element: the launch without a map
    assert same_bits(prev[kept], keep_val[kept])                      # a kept element: add_noise
    assert not same_bits(prev[kept], ref_prev[kept])
    assert same_bits(x0, ref_x0)                                      # the model's own x0, everywhere
    if v["hist"]:
        assert same_bits(hist, ref_hist) and same_bits(hist, x0)
    else:
        assert same_bits(eps_out, ref_eps)


def test_step_keep_nan_eps_in_kept_pixels_stays_out_of_prev(dev):
    t = _step_case(dev, True, pag=False, hist=True, noise=True, fac=False, seed=1)
    kept_px = (t["map"] <= THR)                                       # (B, HW)
    clean_prev, _, _, _ = _run_step(t, True, keep_coef=torch.tensor([THR, 0.62, 0.78, 0.0], device=dev))
    eps = t["eps"].clone().view(2, B, HW, 8)                          # [uncond; cond] rows
    nan16 = torch.tensor([0x7E00, 0x7C01, 0xFE00, 0x7C00], dtype=torch.int32).to(torch.int16).view(torch.float16).to(dev)
    pattern = nan16[torch.arange(8, device=dev) % 4]                  # quiet / signalling NaN and Inf bit patterns
    eps[:, kept_px] = pattern
    t["eps"] = eps.view(-1, 8)
    prev, x0, _, _ = _run_step(t, True, keep_coef=torch.tensor([THR, 0.62, 0.78, 0.0], device=dev))
    kept = kept_px.reshape(B, 1, H, W).expand(B, C, H, W)
    assert not torch.isfinite(x0[kept]).any()                         # the poison is there ...
    assert torch.isfinite(prev).all() and same_bits(prev, clean_prev)      # ... and never reaches prev


def test_step_keep_final_pair_returns_lq_bits(dev):
    t = _step_case(dev, True, pag=False, hist=False, noise=False, fac=False, seed=2)
    t["lq"].view(-1)[::5] = -0.0                                      # the sign of zero survives too
    t["noise0"].view(-1)[0::3] = float("nan")
    t["noise0"].view(-1)[1::3] = float("inf")
    t["noise0"].view(-1)[2::3] = -float("inf")
    ref_prev, _, _, _ = _run_step(t, True)
    prev, _, _, _ = _run_step(t, True, keep_coef=torch.tensor([THR, 1.0, 0.0, 0.0], device=dev))
    kept = (t["map"] <= THR).reshape(B, 1, H, W).expand(B, C, H, W)
    assert same_bits(prev[kept], t["lq"][kept]) and same_bits(prev[~kept], ref_prev[~kept])


def test_step_keep_refuses_bad_keep_tensors(dev):
    from instantir_amd import ops
    t = _step_case(dev, True, pag=False, hist=False, noise=False, fac=False)
    prev = torch.empty_like(t["x"])
    kcoef = torch.tensor([THR, 1.0, 0.0, 0.0], device=dev)
    with pytest.raises(ValueError, match="keep map"):
        ops.sched_step(t["eps"], B, t["coef"], t["x"], prev, keep=(t["map"][:1], t["lq"], t["noise0"], kcoef))
    with pytest.raises(ValueError, match="keep coef"):
        ops.sched_step(t["eps"], B, t["coef"], t["x"], prev, keep=(t["map"], t["lq"], t["noise0"], kcoef.cpu()))
    from instantir_amd.lib import HipLibraryError
    with pytest.raises(HipLibraryError, match="iir_sched_step"):          # keep_src may not be the output
        ops.sched_step(t["eps"], B, t["coef"], t["x"], prev, keep=(t["map"], prev, t["noise0"], kcoef))


# ---- iir_map_pool_max_f32 -----------------------------------------------------------------------------------------
def test_pool_max_equals_max_pool2d(dev):
    from instantir_amd import ops
    g = torch.Generator().manual_seed(3)
    m = torch.rand(2, 24, 40, generator=g)
    m[0, :8, :8] = 0.0
    m[1, 8:16, 32:] = 1.0
    got = ops.map_pool_max(m.to(dev), 8)
    assert got.shape == (2, 3, 5)
    assert same_bits(got, torch.nn.functional.max_pool2d(m[:, None], 8)[:, 0])
    assert same_bits(ops.map_pool_max(m.to(dev), 1), m)
    with pytest.raises(ValueError, match="not a multiple"):
        ops.map_pool_max(torch.rand(2, 25, 40, device=dev), 8)


# ---- iir_region_composite_f32 -------------------------------------------------------------------------------------
def _window_counts(P, r):
    """Integer window sums of a 0/1 map (B, H, W) over (2r+1) x (2r+1) with replicate edges, by cumsum."""
    Hh, Ww = P.shape[1:]
    iy = torch.arange(-r, Hh + r).clamp(0, Hh - 1)
    ix = torch.arange(-r, Ww + r).clamp(0, Ww - 1)
    Pp = P.to(torch.int64)[:, iy][:, :, ix]
    k = 2 * r + 1
    cs = torch.nn.functional.pad(Pp.cumsum(2), (1, 0))
    rows = cs[:, :, k:] - cs[:, :, :-k]
    cs = torch.nn.functional.pad(rows.cumsum(1), (0, 0, 1, 0))
    return cs[:, k:] - cs[:, :-k]


def composite_restatement(decoded, original, map_px, r):
    """The contract's formula in torch (CPU, fp32, one rounding per operation, no FMA)."""
    cnt = _window_counts(map_px > 0, r)
    n2 = (2 * r + 1) ** 2
    w = (cnt.to(torch.float32) / torch.full(cnt.shape, float(n2), dtype=torch.float32))[:, None]
    mix = w * decoded + (1.0 - w) * original
    cnt = cnt[:, None].expand_as(decoded)
    return torch.where(cnt == n2, decoded, torch.where(cnt == 0, original, mix)), cnt


def _composite_inputs(Hh, Ww, seed):
    g = torch.Generator().manual_seed(seed)
    dec, orig = torch.rand(2, 3, Hh, Ww, generator=g), torch.rand(2, 3, Hh, Ww, generator=g)
    m = torch.zeros(2, Hh, Ww)
    m[0, :, Ww // 2:] = torch.rand(Hh, Ww - Ww // 2, generator=g) * 0.9 + 0.1           # a half plane of any positive strength
    m[1] = (torch.rand(Hh, Ww, generator=g) > 0.8).float()                              # scattered pixels: every count occurs
    m[1, :3, :3] = 1.0
    return dec, orig, m


@pytest.mark.parametrize("Hh, Ww, r", [(37, 53, 0), (37, 53, 1), (37, 53, 4), (16, 16, 40)])
def test_composite_equals_restatement(dev, Hh, Ww, r):
    from instantir_amd import ops
    dec, orig, m = _composite_inputs(Hh, Ww, 10 + r)
    want, cnt = composite_restatement(dec, orig, m, r)
    got = ops.region_composite(dec.to(dev), orig.to(dev), m.to(dev), r)
    torch.cuda.synchronize()
    assert same_bits(got, want)
    inplace = dec.to(dev).clone()
    assert ops.region_composite(inplace, orig.to(dev), m.to(dev), r, out=inplace) is inplace       # out == decoded
    torch.cuda.synchronize()
    assert same_bits(inplace, want)
    # kept-exact and changed-exact, stated without the counts: image 0 is free on columns >= W // 2
    x0 = Ww // 2
    if x0 - r > 0:
        assert same_bits(got[0, :, :, :x0 - r], orig[0, :, :, :x0 - r])               # farther than r from the free half
        assert same_bits(got[0, :, :, x0 + r:], dec[0, :, :, x0 + r:])
    if r:
        seam = (cnt > 0) & (cnt < (2 * r + 1) ** 2)                   # and the seam is a true mix
        assert seam.any() and not same_bits(got.cpu()[seam], dec[seam]) and not same_bits(got.cpu()[seam], orig[seam])


def test_composite_refuses_mismatched_inputs(dev):
    from instantir_amd import ops
    dec, orig, m = (t.to(dev) for t in _composite_inputs(16, 16, 1))
    with pytest.raises(ValueError, match="feather"):
        ops.region_composite(dec, orig, m, -1)
    with pytest.raises(ValueError, match="do not match"):
        ops.region_composite(dec, orig[:, :, :8].contiguous(), m, 1)
    with pytest.raises(ValueError, match="do not match"):
        ops.region_composite(dec, orig, m[:1].contiguous(), 1)


# ---- the loop -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def env(dev):
    cfg, sd, sda, lora, inp = lr.tiny_env(noises=N_STEPS)
    Hl = inp["H"]
    # two different maps: every threshold of the 6-step table occurs as a value (with its neighbours), plus 0, 0.3 and 1
    thr = torch.tensor([(N_STEPS - 1 - i) / N_STEPS for i in range(N_STEPS)], dtype=torch.float32)
    vals = torch.cat([thr, torch.nextafter(thr, torch.tensor(1.0)), torch.tensor([0.0, 0.3, 1.0, 1.0])])
    m = torch.stack([vals[(torch.arange(Hl * Hl) * 7 + s) % len(vals)].reshape(Hl, Hl) for s in (0, 5)])[:, None]
    inp["map"] = m
    inp["map2"] = torch.stack([m[1, 0].t(), m[0, 0].flip(0)])[:, None].contiguous()
    return cfg, sd, sda, lora, inp


def _pipe(env, sched):
    pipe = lr.pipe(env, sched)
    assert pipe.use_graphs                                            # hipGraph capture is the default, and stays on here
    return pipe


_call = functools.partial(lr.call, num_inference_steps=N_STEPS, guidance_scale=5.0)


def _contract_callback(inp, m, dev, seen):
    """The contract of DESIGN.md section 7, applied after every step in torch: the yardstick a caller could build before."""
    lq, n0, mp = inp["lq"].to(dev), inp["init_noise"].to(dev), m.to(dev)

    def cb(pipe, i, t, kw):
        x = kw["latents"]
        ts = pipe.scheduler.timesteps
        n = len(ts)
        thr = torch.tensor((n - 1 - i) / n, dtype=torch.float32, device=dev)
        keep = lq if i == n - 1 else pipe.scheduler.add_noise(lq, n0, torch.stack([ts[i + 1]] * lq.shape[0]))
        kept = (mp <= thr).expand_as(x)
        seen.append(int(kept.sum()))
        return {"latents": torch.where(kept, keep, x)}
    return cb


def _schedulers():
    from instantir_amd.schedulers import DDIMScheduler, DDPMScheduler, DPMSolverMultistepScheduler, EulerAncestralDiscreteScheduler
    return {"ddpm": (DDPMScheduler, True), "ddim": (DDIMScheduler, False), "euler_a": (EulerAncestralDiscreteScheduler, True),
            "dpmpp_2m": (DPMSolverMultistepScheduler, False)}


@pytest.mark.parametrize("name", ["ddpm", "ddim", "euler_a", "dpmpp_2m"])
def test_fused_map_equals_the_callback_contract(env, dev, name):
    cls, noisy = _schedulers()[name]
    inp = env[4]
    kw = dict(step_noises=inp["noises"]) if noisy else {}
    fused = _call(_pipe(env, cls()), inp, restore_map=inp["map"], **kw)
    seen = []
    by_callback = _call(_pipe(env, cls()), inp, callback_on_step_end=_contract_callback(inp, inp["map"], dev, seen), **kw)
    assert len(seen) == N_STEPS and len(set(seen)) == N_STEPS and seen[-1] > 0        # another set of pixels every step
    assert torch.isfinite(fused).all()
    assert same_bits(fused, by_callback)
    plain = _call(_pipe(env, cls()), inp, **kw)
    assert not same_bits(fused, plain)
    never = (inp["map"] == 0).expand_as(fused)
    assert same_bits(fused[never], inp["lq"][never])                  # s = 0 comes out as the LQ latent


def test_map_endpoints(env, dev):
    from instantir_amd.schedulers import DDPMScheduler
    inp = env[4]
    kw = dict(step_noises=inp["noises"])
    plain = _call(_pipe(env, DDPMScheduler()), inp, **kw)
    ones = _call(_pipe(env, DDPMScheduler()), inp, restore_map=torch.ones(16, 16), **kw)
    zeros = _call(_pipe(env, DDPMScheduler()), inp, restore_map=torch.zeros(2, 1, 16, 16), **kw)
    assert same_bits(ones, plain)
    assert same_bits(zeros, inp["lq"]) and not same_bits(plain, inp["lq"])


def test_cached_loop_serves_map_no_map_and_another_map(env, dev):
    """One pipeline (IIR_LOOP_CACHE default): a map, no map, another map on the same geometry -- each equal to a fresh pipeline."""
    from instantir_amd.schedulers import DDIMScheduler
    assert os.environ.get("IIR_LOOP_CACHE", "1") != "0"
    inp = env[4]
    pipe = _pipe(env, DDIMScheduler())
    seq = [dict(restore_map=inp["map"]), {}, dict(restore_map=inp["map2"]), dict(restore_map=inp["map"])]
    got = [_call(pipe, inp, **kw) for kw in seq]
    assert pipe._loop_cache is not None and pipe._loop_cache[1].masked
    for kw, g in zip(seq[:3], got):
        assert same_bits(g, _call(_pipe(env, DDIMScheduler()), inp, **kw)), list(kw)
    assert same_bits(got[3], got[0]) and not same_bits(got[2], got[0])


def test_call_refuses_bad_maps(env, dev):
    from instantir_amd.schedulers import DDIMScheduler
    inp = env[4]
    pipe = _pipe(env, DDIMScheduler())
    with pytest.raises(ValueError, match=r"must lie in \[0, 1\]"):
        _call(pipe, inp, restore_map=torch.full((16, 16), 1.01))
    with pytest.raises(ValueError, match="non-finite"):
        _call(pipe, inp, restore_map=torch.full((16, 16), float("nan")))
    with pytest.raises(ValueError, match=r"must match the image \(128, 128\) or the latent \(16, 16\)"):
        _call(pipe, inp, restore_map=torch.zeros(32, 32))
    with pytest.raises(ValueError, match="map_feather"):
        _call(pipe, inp, restore_map=torch.zeros(16, 16), map_feather=-1)
    # a pixel-size map on a latent `image`: pooled to the latent, no composite (there are no input pixels)
    px = torch.nn.functional.interpolate(inp["map"], scale_factor=8, mode="nearest")
    assert same_bits(_call(pipe, inp, restore_map=px), _call(pipe, inp, restore_map=inp["map"]))


# ---- pixels in, pixels out ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def penv(dev):
    from instantir_amd import weights as Wt
    from instantir_amd.config import UNetConfig, VAEConfig
    from instantir_amd.pipeline import InstantIRPipeline
    from instantir_amd.schedulers import DDIMScheduler, LCMSingleStepScheduler
    from instantir_amd.vae import HipVAE
    cfg, vc = UNetConfig.tiny(), VAEConfig.tiny()
    vae = HipVAE(vc, Wt.synth_state_dict(Wt.vae_decoder_specs(vc) + Wt.vae_encoder_specs(vc), 21, dtype=torch.bfloat16), dev)
    pipe = InstantIRPipeline(cfg, Wt.synth_state_dict(Wt.unet_specs(cfg), 11), scheduler=DDIMScheduler(), vae=vae, device=dev)
    pipe.aggregator.load_state_dict(Wt.synth_state_dict(Wt.aggregator_specs(cfg), 12))
    pipe.prepare_previewers(Wt.synth_state_dict(Wt.lora_specs(cfg), 13), lora_alpha=8)
    g = torch.Generator().manual_seed(9)
    px = 128
    kw = dict(image=torch.rand(2, 3, px, px, generator=g),
              prompt_embeds=torch.randn(2, cfg.text_len, cfg.cross_attention_dim, generator=g).half().float(),
              pooled_prompt_embeds=torch.randn(2, cfg.pooled_dim, generator=g).half().float(),
              ip_adapter_image_embeds=[torch.randn(2, 2, cfg.resampler.seq_len, cfg.resampler.embedding_dim, generator=g).half().float()],
              vae_noise=torch.randn(2, 4, px // 8, px // 8, generator=g), init_noise=torch.randn(2, 4, px // 8, px // 8, generator=g),
              num_inference_steps=N_STEPS, guidance_scale=5.0, previewer_scheduler=LCMSingleStepScheduler.from_config(pipe.scheduler.config))
    m = torch.zeros(2, 1, px, px)
    m[0, :, :, 64:] = 1.0                                             # image 0: the right half is free
    m[1, :, 64:, :] = 0.6                                             # image 1: the lower half, for part of the schedule
    return pipe, kw, m


@pytest.mark.parametrize("feather, color_fix", [(4, None), (0, None), (4, "wavelet")])
def test_pixels_in_pixels_out(penv, dev, feather, color_fix):
    from instantir_amd import ops
    pipe, kw, m = penv
    out = pipe(output_type="pt", restore_map=m, map_feather=feather, color_fix=color_fix, **kw).images
    assert out.shape == (2, 3, 128, 128) and out.dtype == torch.float32
    # the prepared image mapped to [0, 1]: the tensor the colour fix takes as its reference
    original = ((kw["image"] * 2.0 - 1.0) / 2 + 0.5).clamp(0, 1)
    r = feather
    assert same_bits(out[0, :, :, :64 - r], original[0, :, :, :64 - r])              # farther than r from the free half: the input
    assert same_bits(out[1, :, :64 - r, :], original[1, :, :64 - r, :])
    # the same call's decode without the composite: its final latents through the VAE (and the colour fix)
    lat = pipe(output_type="latent", restore_map=m, map_feather=feather, **kw).images
    decoded = pipe.vae.decode_latent(lat, "pt").contiguous()
    if color_fix is not None:
        decoded = ops.colorfix(decoded, original.to(dev).contiguous(), color_fix)
    torch.cuda.synchronize()
    assert same_bits(out[0, :, :, 64 + r:], decoded[0, :, :, 64 + r:])               # the free half, away from the seam
    assert same_bits(out[1, :, 64 + r:, :], decoded[1, :, 64 + r:, :])
    assert not same_bits(decoded[0, :, :, :64 - r], original[0, :, :, :64 - r])      # a VAE round trip is not the input
    if r:
        seam = out[0, :, :, 64 - r:64 + r].cpu()
        assert not same_bits(seam, decoded[0, :, :, 64 - r:64 + r]) and not same_bits(seam, original[0, :, :, 64 - r:64 + r])
    # a latent-size map has no pixels to feather
    with pytest.raises(ValueError, match="latent size"):
        pipe(output_type="pt", restore_map=torch.ones(16, 16), **kw)
    # ... but serves a call that stops at the latent; and the preview row is never composited
    assert same_bits(pipe(output_type="latent", restore_map=torch.nn.functional.max_pool2d(m, 8), **kw).images, lat)


def test_preview_row_is_not_composited(penv, dev):
    pipe, kw, m = penv
    _, rows0 = pipe(output_type="pt", return_dict=False, save_preview_row=True, restore_map=m, map_feather=0, **kw)
    lat, rows_lat = pipe(output_type="latent", return_dict=False, save_preview_row=True, restore_map=m, **kw)
    assert len(rows0) == len(rows_lat) > 0
    original = ((kw["image"] * 2.0 - 1.0) / 2 + 0.5).clamp(0, 1)
    for a, b in zip(rows0, rows_lat):
        assert same_bits(a, pipe.vae.decode_latent(b, "pt"))
        assert not same_bits(a[0, :, :, :60], original[0, :, :, :60])


# ---- CLI ----------------------------------------------------------------------------------------------------------
def test_cli_restore_map_keeps_the_input_pixels(dev, tmp_path):
    from PIL import Image
    import instantir_amd.infer as cli
    src, out = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    rng = np.random.default_rng(0)
    Image.fromarray(rng.integers(0, 255, (96, 96, 3), dtype=np.uint8)).save(src / "a.png")
    mask = np.zeros((96, 96), dtype=np.uint8)
    mask[:, 48:] = 255                                                # the right half is restored, the left half kept
    Image.fromarray(mask).save(tmp_path / "map.png")
    args = cli.build_parser().parse_args(["--test_path", str(src), "--out_path", str(out), "--synthetic", "tiny", "--num_inference_steps", "2",
                                          "--width", "128", "--height", "128", "--cfg", "5.0", "--restore_map", str(tmp_path / "map.png"),
                                          "--map_feather", "2"])
    orig = cli.resize_img
    cli.resize_img = lambda im, **kw: orig(im, max_side=128, min_side=128, **kw)      # keep the tiny nets tiny
    try:
        cli.main(args, dev)
    finally:
        cli.resize_img = orig
    got = np.asarray(Image.open(out / "a.png"))
    resized, _ = orig(Image.open(src / "a.png").convert("RGB"), max_side=128, min_side=128, width=128, height=128)
    want = np.asarray(resized)                                        # uint8, as the CLI's own conversion of its output
    map128 = np.asarray(Image.open(tmp_path / "map.png").convert("L").resize([128, 128], Image.BILINEAR))
    first_free = int(np.argmax(map128.max(axis=0) > 0))               # the first column the resized map frees
    assert 56 <= first_free <= 66
    assert got.shape == (128, 128, 3)
    assert np.array_equal(got[:, :first_free - 2], want[:, :first_free - 2])          # kept: the resized input, farther than r
    assert not np.array_equal(got[:, 72:], want[:, 72:])              # restored: not the input
