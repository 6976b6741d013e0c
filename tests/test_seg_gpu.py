"""GPU: smoothed-energy guidance (SEG; Hong 2024) -- iir_seg_blur_q_f16 element-wise against the fp64 restatement of
tests/seg_ref.py, the denoising loop against the CPU fp32 oracle with its self-attention in SEG form (seg_ref.swap_attn_self;
oracle/nets.py is not edited), and the bit-identity of everything SEG must not touch.  Loop geometry, pipelines and the oracles are
those of tests/loop_ref.py."""
import functools
import math
import os

import numpy as np
import pytest
import torch

import seg_ref
import loop_ref as lr
import test_pag_gpu as tp
from loop_ref import dev, env, pag_oracle_attn  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

BAR = tp.BAR                # 60 dB: the bar of test_pag_gpu's loop cases
GAP = 10.0                  # the plain and the PAG'd oracle must each be at least this much further away


# ---- the blur kernel ------------------------------------------------------------------------------------------------------------
# (images, H, W, C, ldq, sigma)
SHAPES = [(1, 8, 8, 64, 128, 1.0), (2, 7, 9, 64, 136, 0.5), (2, 7, 9, 64, 136, 10.0), (2, 8, 12, 72, 144, 2.5),
          (1, 1, 16, 64, 128, 1.0), (1, 2, 2, 8, 16, 3.0), (2, 32, 32, 1280, 2560, 100.0), (1, 64, 64, 640, 1280, 2.0),
          (1, 128, 128, 64, 128, 4.0)]
MEAN_SHAPES = [(2, 7, 9, 64, 136, math.inf), (2, 32, 32, 1280, 2560, 1e4), (1, 128, 128, 64, 128, math.inf)]
ROWS_BEFORE, ROWS_AFTER = 3, 2
_ids = lambda s: "x".join(str(v) for v in s)


def _buffer(shape, seed=0):
    """The q | k buffer around the perturbed rows: ROWS_BEFORE rows of other batch rows, images * H * W rows whose columns [0, C)
    are Q, [C, 2C) (as far as ldq reaches) K, anything beyond NaN bit patterns; ROWS_AFTER rows of NaN bit patterns behind."""
    images, H, W, C, ldq, _ = shape
    g = torch.Generator().manual_seed(seed + images * 7 + H * 131 + W * 17 + C)
    M = images * H * W
    buf = (torch.randn(ROWS_BEFORE + M + ROWS_AFTER, ldq, generator=g) * 1.5).half()
    nan = torch.tensor([0x7E00, 0x7C01, -1, 0x7FFF], dtype=torch.int16).view(torch.half)         # quiet, signalling, negative NaNs
    fill = lambda t: t.copy_(nan.repeat((t.numel() + 3) // 4)[:t.numel()].view(t.shape))
    fill(buf[ROWS_BEFORE + M:])
    if ldq > 2 * C:
        fill(buf[:, 2 * C:])
    return buf


def _run(buf, shape, dev):
    from instantir_amd import ops, seg
    images, H, W, C, ldq, sigma = shape
    d = buf.to(dev)
    q = d[ROWS_BEFORE:ROWS_BEFORE + images * H * W, :C]
    if seg.is_mean(sigma):
        ops.seg_blur_q(q, images, H, W, mean=True)
    else:
        tap = lambda n: torch.tensor(seg.weights(sigma, n), dtype=torch.float64).float().to(dev)
        ops.seg_blur_q(q, images, H, W, tap(H), tap(W))
    torch.cuda.synchronize()
    return d.cpu()


def _check(shape, dev):
    images, H, W, C, ldq, sigma = shape
    buf = _buffer(shape)
    out = _run(buf, shape, dev)
    M, T = images * H * W, H * W
    q = buf[ROWS_BEFORE:ROWS_BEFORE + M, :C].double().view(images, H, W, C)
    got = out[ROWS_BEFORE:ROWS_BEFORE + M, :C].double().view(images, H, W, C)
    ref = seg_ref.seg_q(q, sigma)
    # containment: everything but Q's columns of the perturbed rows keeps its bits (K, the rows before, the NaN guard bands)
    keep = torch.ones(buf.shape, dtype=torch.bool)
    keep[ROWS_BEFORE:ROWS_BEFORE + M, :C] = False
    assert torch.equal(out.view(torch.int16)[keep], buf.view(torch.int16)[keep])
    assert torch.isfinite(got).all()
    # |out - ref| <= 2^-11 |ref| (the one fp16 rounding) + n 2^-24 max|q| (fp32 sums of a convex combination) + 2^-25 (subnormal
    # floor); n = ky + kx + 2 for the blur; the mean is a pairwise TREE over the T tokens: n = log2(T) + 2
    n = (math.log2(T) + 2) if seg_ref.is_mean(sigma) else (seg_ref.kernel_length(sigma, H) + seg_ref.kernel_length(sigma, W) + 2)
    bound = 2.0 ** -11 * ref.abs() + n * 2.0 ** -24 * q.abs().max().item() + 2.0 ** -25
    err = (got - ref).abs()
    worst = (err / bound).max().item()
    print(f"{_ids(shape)}: max |out - ref| {err.max().item():.3e}, worst error / bound {worst:.3f}")
    assert worst <= 1.0, worst
    return buf, out


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_blur_matches_fp64(dev, shape):
    _check(shape, dev)


@pytest.mark.parametrize("shape", MEAN_SHAPES, ids=_ids)
def test_mean_mode_matches_fp64(dev, shape):
    _check(shape, dev)


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[3], SHAPES[8], MEAN_SHAPES[0]], ids=_ids)
def test_images_do_not_bleed_and_launches_repeat(dev, shape):
    """Changing image 1 (or, with one image, the rows before and K) leaves image 0's output bits alone; two launches on equal
    inputs give equal bits."""
    images, H, W, C, ldq, _ = shape
    buf = _buffer(shape)
    a, b = _run(buf, shape, dev), _run(buf, shape, dev)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    other = buf.clone()
    T = H * W
    if images > 1:
        other[ROWS_BEFORE + T:ROWS_BEFORE + images * T, :C] = other[ROWS_BEFORE + T:ROWS_BEFORE + images * T, :C].flip(0) * 2
    other[:ROWS_BEFORE] = 7.0
    other[ROWS_BEFORE:ROWS_BEFORE + images * T, C:min(2 * C, ldq)] = -3.0
    c = _run(other, shape, dev)
    first = (slice(ROWS_BEFORE, ROWS_BEFORE + T), slice(0, C))
    assert torch.equal(a[first].view(torch.int16), c[first].view(torch.int16))
    if images > 1:
        assert not torch.equal(a[ROWS_BEFORE + T:ROWS_BEFORE + 2 * T, :C], c[ROWS_BEFORE + T:ROWS_BEFORE + 2 * T, :C])


def test_ops_wrapper_refuses_bad_arguments(dev):
    from instantir_amd import ops
    from instantir_amd.lib import HipLibraryError
    q = torch.zeros(64, 128, dtype=torch.half, device=dev)
    w3 = torch.tensor([0.25, 0.5, 0.25], device=dev)
    with pytest.raises(ValueError, match="rows"):
        ops.seg_blur_q(q[:, :64], 1, 8, 9, w3, w3)
    with pytest.raises(ValueError, match="wy"):
        ops.seg_blur_q(q[:, :64], 1, 8, 8, None, w3)
    with pytest.raises(ValueError, match="wx"):
        ops.seg_blur_q(q[:, :64], 1, 8, 8, w3, w3.double())
    with pytest.raises(HipLibraryError):
        ops.seg_blur_q(q[:, :64], 1, 8, 8, w3, w3[:2].contiguous())          # an even kernel: refused by the entry


# ---- the denoising loop ------------------------------------------------------------------------------------------------------------
@pytest.fixture
def seg_oracle_attn(monkeypatch, pag_oracle_attn):
    """oracle.nets.attn_self in SEG form (over the PAG'd form, so that one test can build both oracles)."""
    seg_ref.swap_attn_self(monkeypatch)
    yield
    seg_ref.SEG["paths"] = None


_call = functools.partial(lr.call, **lr.LOOP)


def _check_loop(tag, got, want, plain, pagd):
    o_plain, o_pag = lr.psnr(plain, want), lr.psnr(pagd, want)
    print(f"{tag}: the SEG'd oracle is {o_plain:.1f} dB from the plain oracle and {o_pag:.1f} dB from the PAG'd one")
    assert o_plain <= BAR - GAP and o_pag <= BAR - GAP, (o_plain, o_pag)      # on CPU values alone: a no-op or PAG-like blur cannot pass
    p, p_plain, p_pag = lr.psnr(got, want, "seg." + tag), lr.psnr(got, plain), lr.psnr(got, pagd)
    print(f"{tag}: latent PSNR vs SEG'd oracle {p:.1f} dB, vs plain oracle {p_plain:.1f} dB, vs PAG'd oracle {p_pag:.1f} dB")
    assert torch.isfinite(got).all() and p >= BAR, p
    assert p_plain <= p - GAP and p_pag <= p - GAP, (p, p_plain, p_pag)


APG = (0.0, 6.0, -0.5)           # eta, norm_threshold, momentum: the parameters of test_apg_gpu's loop tests
# name -> (call arguments, layers, seg_blur_sigma, APG parameters).  seg_blur_sigma stays at its default 100.  seg_scale: the
# tiny `mid` block runs on 4 x 4 tokens and moves eps little, so at the default scale 3 the SEG'd oracle is only 53.6 - 55.8 dB
# from the plain one (41.1 - 43.4 from the PAG'd one) -- too close to show a 10 dB gap under a 60 dB bar.  From these CPU values
# alone the scale of the `mid` cases was raised to 6, where every reference pair is at most 49.9 dB apart (BAR - GAP = 50;
# `_check_loop` asserts that too); `up_blocks.0` separates at 3 (44.6 / 31.8 dB).
CASES = {
    "cfg7_mid": (dict(guidance_scale=7.0, seg_scale=6.0), "mid", 100.0, None),
    "cfg1_up0": (dict(guidance_scale=1.0, seg_scale=3.0), "up_blocks.0", 100.0, None),
    "rescale": (dict(guidance_scale=7.0, seg_scale=6.0, guidance_rescale=0.7), "mid", 100.0, None),
    "apg": (dict(guidance_scale=7.0, seg_scale=6.0), "mid", 100.0, APG),
    "sigma_inf": (dict(guidance_scale=7.0, seg_scale=6.0), "mid", math.inf, None),
}


def _seg_pipe(env, layers, sigma=100.0, sched=None, apg=None):
    pipe = lr.pipe(env, sched)
    pipe.enable_seg(layers, seg_blur_sigma=sigma)
    if apg is not None:
        pipe.enable_apg(*apg)
    return pipe


@pytest.mark.parametrize("case", sorted(CASES))
def test_loop_matches_seg_oracle(env, seg_oracle_attn, case):
    """Eight DDIM steps through every phase (Aggregator-only head, previewed middle, creative tail): >= 60 dB against the SEG'd
    oracle, and the plain oracle and the PAG'd oracle of the same layers each at least 10 dB further away."""
    call_kw, layers, sigma, apg = CASES[case]
    g, s, phi = call_kw["guidance_scale"], call_kw["seg_scale"], call_kw.get("guidance_rescale", 0.0)
    want = lr.guided(env, "seg", layers, guidance_scale=g, scale=s, sigma=sigma, guidance_rescale=phi, apg_par=apg)
    plain = lr.guided(env, None, guidance_scale=g, guidance_rescale=phi, apg_par=apg)
    pagd = lr.guided(env, "pag", layers, guidance_scale=g, scale=s, guidance_rescale=phi, apg_par=apg)
    got = _call(_seg_pipe(env, layers, sigma, apg=apg), env[4], **call_kw)
    _check_loop(case, got, want, plain, pagd)


def test_dpmpp_2m_karras_matches_seg_oracle(env, seg_oracle_attn):
    """The sigma-scheduler oracle loop (DPM++ 2M Karras) with the hooks of the DDIM cases."""
    from instantir_amd import pag
    g, s = 5.0, 6.0                  # (the scale of the `mid` cases: see CASES)
    paths, B = pag.select("mid", pag.attn1_paths(env[0])), env[4]["B"]
    oracle = functools.partial(lr.sigma_denoise, env, "dpm", 8, guidance_scale=g, karras=True, **lr.PHASES)
    want = oracle(main_unet=lr.seg_unet(paths, B, 100.0), guide=lr.perturbed(g, s))
    plain = oracle()
    pagd = oracle(main_unet=lr.pag_unet(paths, B), guide=lr.perturbed(g, s))
    got = _call(_seg_pipe(env, "mid", sched=lr.sigma_sched("dpm", karras=True)), env[4], guidance_scale=g, seg_scale=s)
    _check_loop("dpmpp_2m_karras", got, want, plain, pagd)


# ---- bit-identity ------------------------------------------------------------------------------------------------------------------
def test_disabled_and_zero_scale_bit_identical_to_never_enabled(env):
    inp = env[4]
    base = _call(lr.pipe(env), inp)
    p = _seg_pipe(env, "mid")
    p.disable_seg()
    assert torch.equal(_call(p, inp), base)
    p2 = _seg_pipe(env, ["mid", "up_blocks.0"])
    assert torch.equal(_call(p2, inp, seg_scale=0.0), base)
    assert p2._unet.seg is None and p2._unet.pag is None            # scale 0: the plain launches ran


def test_toggling_seg_pag_off_replays_the_right_graphs(env):
    """SEG -> PAG -> off -> SEG -> SEG (other sigma) -> SEG (other scale) on ONE pipeline: each call equals a fresh pipeline in
    that state, bit for bit; the scale alone re-uses the captured loop, sigma and the method do not."""
    inp = env[4]
    settings = [("seg", "mid", 100.0, 3.0), ("pag", "mid", None, 3.0), None, ("seg", "mid", 100.0, 3.0), ("seg", "mid", 1.0, 3.0),
                ("seg", "mid", 1.0, 1.5)]

    def apply(pipe, st):
        pipe.disable_seg()
        pipe.disable_pag()
        if st is None:
            return {}
        if st[0] == "pag":
            pipe.enable_pag(st[1])
            return dict(pag_scale=st[3])
        pipe.enable_seg(st[1], seg_blur_sigma=st[2])
        return dict(seg_scale=st[3])

    fresh = {}
    for st in set(settings):
        f = lr.pipe(env)
        fresh[st] = _call(f, inp, **apply(f, st))
    pipe, loops = lr.pipe(env), []
    for st in settings:
        assert torch.equal(_call(pipe, inp, **apply(pipe, st)), fresh[st]), st
        loops.append(pipe._loop_cache[1])
    assert loops[4] is loops[5] and loops[3] is not loops[4] and loops[0] is not loops[1] and loops[1] is not loops[2]
    assert len({fresh[st].numpy().tobytes() for st in fresh}) == len(fresh)          # five states, five results


def test_graphs_on_off_and_repeat_calls_bit_identical(env):
    inp = env[4]
    pipe = _seg_pipe(env, ["mid", "up_blocks.0"], 2.0)
    a = _call(pipe, inp)
    b = _call(pipe, inp)
    pipe.use_graphs = False
    c = _call(pipe, inp)
    pipe.use_graphs, pipe.overlap_streams = True, False
    d = _call(pipe, inp)
    assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, d)


def test_composes_with_restore_map_adastep_and_callback(env):
    """restore_map, adastep_restore and callback_on_step_end run with SEG: finite, repeatable, and SEG changes the result."""
    inp = env[4]
    rmap = torch.ones(16, 16)
    rmap[:, :8] = 0.0
    seen = []

    def cb(p, i, t, kw):
        seen.append(i)
        return {}
    kw = dict(restore_map=rmap, adastep_restore=True, callback_on_step_end=cb)
    a = _call(_seg_pipe(env, "mid"), inp, **kw)
    b = _call(_seg_pipe(env, "mid"), inp, **kw)
    c = _call(lr.pipe(env), inp, **kw)
    assert torch.isfinite(a).all() and torch.equal(a, b) and not torch.equal(a, c) and seen[:8] == list(range(8))


def test_cli_seg_equals_python_api(tmp_path, dev):
    from PIL import Image
    import instantir_amd.infer as cli
    src, out = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    Image.fromarray(np.random.default_rng(0).integers(0, 255, (96, 96, 3), dtype=np.uint8)).save(src / "a.png")
    args = cli.build_parser().parse_args(["--test_path", str(src), "--out_path", str(out), "--synthetic", "tiny",
                                          "--num_inference_steps", "4", "--width", "128", "--height", "128", "--batch_size", "1",
                                          "--cfg", "5.0", "--seg_scale", "2.5", "--seg_blur_sigma", "1.5",
                                          "--seg_layers", "mid,up_blocks.0"])
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
    pipe.enable_seg(["mid", "up_blocks.0"], seg_blur_sigma=1.5)
    cfg = pipe.cfg
    g = torch.Generator().manual_seed(42)
    kw = dict(prompt_embeds=torch.randn(1, cfg.text_len, cfg.cross_attention_dim, generator=g),
              pooled_prompt_embeds=torch.randn(1, cfg.pooled_dim, generator=g),
              negative_prompt_embeds=torch.randn(1, cfg.text_len, cfg.cross_attention_dim, generator=g),
              negative_pooled_prompt_embeds=torch.randn(1, cfg.pooled_dim, generator=g),
              ip_adapter_image_embeds=[torch.randn(2, 1, cfg.resampler.seq_len, cfg.resampler.embedding_dim, generator=g)])
    rec = pipe(image=[im], num_inference_steps=4, generator=torch.Generator(device=dev).manual_seed(42), guidance_scale=5.0,
               previewer_scheduler=lcm, preview_start=0.0, control_guidance_end=1.0, seg_scale=2.5, **kw).images[0]
    want = np.asarray(rec.resize([size[0], size[1]], Image.BILINEAR))
    assert got.shape == want.shape and np.array_equal(got, want)


def test_grid_beyond_the_blur_limit_is_refused_before_any_launch(env):
    """A selected layer on a grid of more than 128 tokens per axis: ValueError naming the limit (tiny: level 1 of a 264-row latent)."""
    cfg = env[0]
    pipe = _seg_pipe(env, "down_blocks.1")
    B = 1
    g = torch.Generator().manual_seed(0)
    with pytest.raises(ValueError, match="128 x 128"):
        pipe(image=torch.zeros(B, 4, 264, 8), prompt_embeds=torch.randn(B, cfg.text_len, cfg.cross_attention_dim, generator=g),
             pooled_prompt_embeds=torch.randn(B, cfg.pooled_dim, generator=g), guidance_scale=1.0,
             ip_adapter_image_embeds=[torch.randn(1, B, cfg.resampler.seq_len, cfg.resampler.embedding_dim, generator=g)],
             output_type="latent", num_inference_steps=1)


# ---- full size ---------------------------------------------------------------------------------------------------------------------
def test_config1_geometry_one_step_with_seg(dev, seg_oracle_attn):
    """configs[1]'s geometry (1024^2, cfg 7, B = 1, 3 main-UNet rows) for one DDPM step at t = 501 with SEG on `mid` (32 x 32
    tokens, sigma 100: 33 taps per axis), against the SEG'd CPU oracle; two calls bit-identical.  Bar: 50 dB, that of
    test_pag_gpu's full-size case, whose inputs and time budgeting these are."""
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
    pipe.enable_seg("mid")
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
        e = seg_ref.seg_unet(P, cfg, xin, t, ctx, text, tid, ip_main, down, mid, paths, B, 100.0)
        u, c, p = e.chunk(3)
        eps = u + 7.0 * (c - u) + 3.0 * (c - p)
        want, _ = sched.ddpm_step(acp, eps, t, x, 1, noise=sn[0], prev_t=-1)
        plain, _ = sched.ddpm_step(acp, u + 7.0 * (c - u), t, x, 1, noise=sn[0], prev_t=-1)
    v, v_plain = lr.psnr(got, want, "seg.config1_one_step"), lr.psnr(got, plain)
    print(f"configs[1] geometry, one step with SEG (mid): latent PSNR vs CPU fp32 oracle {v:.1f} dB, vs the unguided-by-SEG step {v_plain:.1f} dB")
    assert v >= 50.0, v
