"""GPU: LQ-guided colour fix (color_fix: wavelet, adain) -- the HIP kernels against the fp64 restatement of the contract
(tests/colorfix_ref.py), their determinism, and the pipeline / CLI wiring.

Bounds (set by the contract, not by what the kernels give):
  wavelet: max abs error <= 4e-6.  d = style - content stays in [-1, 1]; ten 3-tap passes with exact (power of two) products
           round at most twice each, plus the first subtraction and the last addition: at most 43 roundings of 2^-24 = 2.6e-6;
           the clamp is 1-Lipschitz; 1.5x on top.
  adain:   max abs error <= max(1e-5, 4 x the error of the same restatement run in fp32 torch on the CPU against fp64 on the
           same inputs).  Both errors go to the measurement log conftest.record_psnr keeps, in units of 1e-9
           (it prints two decimals), and are printed in full, so the bound can be tightened later.
Inputs: the seeded recipe of colorfix_ref.recipe (content = rand, style = a blurred, colour-shifted, noised copy).  For adain
the recipe's noise term is 0.4 instead of 0.05: with 0.05 the style's per-channel std is 0.043 (0.7 * 0.289 / 5 from the 5x5
mean, plus the noise), under the 0.05 the adain inputs must have; the test asserts the std of both inputs.
No test passes on saturated data: at most 10 % of the restated output is exactly 0 or 1 and mean |result - content| > 0.02."""
import pytest
import torch

import colorfix_ref as R

pytestmark = pytest.mark.gpu

WAVELET_BOUND = 4e-6
ADAIN_FLOOR = 1e-5
# B per size: 1 to 3
CASES = [(3, 5, 7), (2, 8, 8), (3, 24, 40), (2, 257, 131), (1, 768, 1024), (2, 1024, 1024), (1, 2048, 2048)]
IDS = [f"{b}x{h}x{w}" for b, h, w in CASES]


def _log(line, **errors):
    """Print the line; `errors` (name -> max abs error) also go to the suite's measurement log, in units of 1e-9."""
    from conftest import record_psnr
    tag = "colorfix." + "_".join(line.split()[:2])
    for name, err in errors.items():
        record_psnr(f"{tag}.{name}_1e-9", err * 1e9)
    print(line)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from instantir_amd import lib
    lib.load()
    return torch.device("cuda:0")


def _inputs(mode, B, H, W, seed=7):
    return R.recipe(B, H, W, seed, noise=0.4 if mode == "adain" else 0.05)


def _guards(want, content):
    sat, moved = R.saturated_fraction(want), (want - content.double()).abs().mean().item()
    assert sat <= 0.10, f"restated output is saturated: {sat:.3f} of it is exactly 0 or 1"
    assert moved > 0.02, f"the restatement barely moves the image: mean |result - content| = {moved:.4f}"
    return sat, moved


def _adain_bound(content, style, want):
    e32 = (R.adain(content, style).double() - want).abs().max().item()
    return max(ADAIN_FLOOR, 4 * e32), e32


# ---- kernels against the fp64 restatement ------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W", CASES, ids=IDS)
def test_wavelet_matches_fp64_restatement(dev, B, H, W):
    from instantir_amd import ops
    content, style = _inputs("wavelet", B, H, W)
    want = R.wavelet(content.double(), style.double())
    sat, moved = _guards(want, content)
    got = ops.colorfix(content.to(dev), style.to(dev), "wavelet")
    torch.cuda.synchronize()
    err = (got.cpu().double() - want).abs().max().item()
    _log(f"wavelet {B}x3x{H}x{W} max_abs_err {err:.3e} bound {WAVELET_BOUND:.1e} saturated {sat:.3f} moved {moved:.3f}",
         max_abs_err=err)
    assert got.shape == content.shape and err <= WAVELET_BOUND, err


@pytest.mark.parametrize("B,H,W", CASES, ids=IDS)
def test_adain_matches_fp64_restatement(dev, B, H, W):
    from instantir_amd import ops
    content, style = _inputs("adain", B, H, W)
    for name, t in (("content", content), ("style", style)):
        assert t.reshape(B, 3, -1).std(2).min().item() >= 0.05, name
    want = R.adain(content.double(), style.double())
    sat, moved = _guards(want, content)
    bound, e32 = _adain_bound(content, style, want)
    got = ops.colorfix(content.to(dev), style.to(dev), "adain")
    torch.cuda.synchronize()
    err = (got.cpu().double() - want).abs().max().item()
    _log(f"adain {B}x3x{H}x{W} max_abs_err {err:.3e} fp32_torch_cpu_err {e32:.3e} bound {bound:.1e} saturated {sat:.3f} moved {moved:.3f}",
         max_abs_err=err, fp32_torch_cpu_err=e32)
    assert err <= bound, (err, bound)


def test_other_channel_counts_and_unaligned_views(dev):
    """C is a launch argument (1 and 4 channels), and a base that is not 16-byte aligned takes the scalar path."""
    from instantir_amd import ops
    g = torch.Generator().manual_seed(2)
    for C, H, W in ((1, 40, 64), (4, 33, 16)):
        c = torch.rand(2, C, H, W, generator=g)
        s = (0.5 * c + 0.3 * torch.rand(2, C, 1, 1, generator=g) + 0.1 * torch.rand(2, C, H, W, generator=g)).clamp(0, 1)
        flat_c, flat_s = torch.zeros(c.numel() + 1, device=dev), torch.zeros(c.numel() + 1, device=dev)
        cu, su = flat_c[1:].view(c.shape), flat_s[1:].view(c.shape)          # 4-byte aligned only
        cu.copy_(c); su.copy_(s)
        assert cu.data_ptr() % 16 == 4 and cu.is_contiguous()
        for mode, bound in (("wavelet", WAVELET_BOUND), ("adain", None)):
            want = R.apply(c.double(), s.double(), mode)
            if bound is None:
                bound = _adain_bound(c, s, want)[0]
            for cc, ss in ((c.to(dev), s.to(dev)), (cu, su)):
                got = ops.colorfix(cc, ss, mode)
                torch.cuda.synchronize()
                assert (got.cpu().double() - want).abs().max().item() <= bound, (mode, C)


def test_wrapper_checks(dev):
    from instantir_amd import ops
    c = torch.rand(1, 3, 8, 8, device=dev)
    with pytest.raises(ValueError, match="mode"):
        ops.colorfix(c, c, "histogram")
    with pytest.raises(ValueError, match="style"):
        ops.colorfix(c, c[:, :, :4], "wavelet")
    with pytest.raises(ValueError, match="fp32"):
        ops.colorfix(c.half(), c.half(), "wavelet")
    with pytest.raises(ValueError, match="contiguous"):
        ops.colorfix(c.permute(0, 1, 3, 2), c, "wavelet")
    with pytest.raises(ValueError, match="2 pixels"):
        ops.colorfix(c[:, :, :1, :1].contiguous(), c[:, :, :1, :1].contiguous(), "adain")
    with pytest.raises(ValueError, match="workspace"):
        ops.colorfix(c, c, "wavelet", ws=torch.empty(16, dtype=torch.uint8, device=dev))
    one = torch.rand(1, 3, 1, 1, device=dev)
    assert torch.equal(ops.colorfix(one, one, "wavelet"), one)             # H = W = 1 is a valid wavelet input


# ---- determinism -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["wavelet", "adain"])
@pytest.mark.parametrize("B,H,W", [(3, 5, 7), (2, 257, 131), (1, 1024, 1024)], ids=["3x5x7", "2x257x131", "1x1024x1024"])
def test_in_place_repeat_and_busy_neighbour_give_the_same_bits(dev, mode, B, H, W):
    from instantir_amd import ops
    content, style = _inputs(mode, B, H, W, seed=11)
    c, s = content.to(dev), style.to(dev)
    first = ops.colorfix(c, s, mode)
    again = ops.colorfix(c, s, mode)
    inplace = c.clone()
    assert ops.colorfix(inplace, s, mode, out=inplace) is inplace
    torch.cuda.synchronize()
    assert torch.equal(first, again), "two runs differ"
    assert torch.equal(first, inplace), "in place differs from out of place"
    assert torch.equal(c.cpu(), content), "content was modified by an out-of-place call"
    # beside a busy second stream
    side = torch.cuda.Stream()
    a = torch.randn(2048, 2048, device=dev, dtype=torch.half)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(24):
            a = (a @ a).clamp_(-1, 1)
    busy = ops.colorfix(c, s, mode)
    torch.cuda.synchronize()
    assert torch.equal(first, busy), "a run beside a busy stream differs"


# ---- pipeline ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def penv(dev):
    from instantir_amd import weights as W
    from instantir_amd.config import UNetConfig, VAEConfig
    from instantir_amd.pipeline import InstantIRPipeline
    from instantir_amd.schedulers import DDIMScheduler, LCMSingleStepScheduler
    from instantir_amd.vae import HipVAE
    cfg, vc = UNetConfig.tiny(), VAEConfig.tiny()
    vae = HipVAE(vc, W.synth_state_dict(W.vae_decoder_specs(vc) + W.vae_encoder_specs(vc), 21, dtype=torch.bfloat16), dev)
    pipe = InstantIRPipeline(cfg, W.synth_state_dict(W.unet_specs(cfg), 11), scheduler=DDIMScheduler(), vae=vae, device=dev)
    pipe.aggregator.load_state_dict(W.synth_state_dict(W.aggregator_specs(cfg), 12))
    pipe.prepare_previewers(W.synth_state_dict(W.lora_specs(cfg), 13), lora_alpha=8)
    return cfg, pipe, LCMSingleStepScheduler.from_config(pipe.scheduler.config)


def _call_kw(cfg, lcm, n_prompt, n_img, nipp, guidance, seed=9, px=128):
    g = torch.Generator().manual_seed(seed)
    B = n_prompt * nipp
    cfg_on = guidance > 1
    return dict(image=torch.rand(n_img, 3, px, px, generator=g),
                prompt_embeds=torch.randn(n_prompt, cfg.text_len, cfg.cross_attention_dim, generator=g).half().float(),
                pooled_prompt_embeds=torch.randn(n_prompt, cfg.pooled_dim, generator=g).half().float(),
                ip_adapter_image_embeds=[torch.randn(2 if cfg_on else 1, n_prompt, cfg.resampler.seq_len, cfg.resampler.embedding_dim,
                                                     generator=g).half().float()],
                vae_noise=torch.randn(n_img, 4, px // 8, px // 8, generator=g), init_noise=torch.randn(B, 4, px // 8, px // 8, generator=g),
                num_inference_steps=2, guidance_scale=guidance, num_images_per_prompt=nipp, previewer_scheduler=lcm)


def _reference_of(image, B, nipp):
    """The default reference as the pipeline documents it: `_prepare_image(image)` mapped back to [0, 1], expanded as lq is."""
    ref = ((image * 2.0 - 1.0) / 2 + 0.5).clamp(0, 1)
    return ref.repeat(B, 1, 1, 1) if ref.shape[0] == 1 else ref.repeat_interleave(nipp, 0)


def _check_against_restatement(got, base, ref, mode, tag):
    want = R.apply(base.double(), ref.double(), mode)
    moved = (want - base.double()).abs().mean().item()
    sat = R.saturated_fraction(want)
    bound = WAVELET_BOUND if mode == "wavelet" else _adain_bound(base, ref, want)[0]
    err = (got.double() - want).abs().max().item()
    _log(f"pipeline {tag} {mode} {tuple(base.shape)} max_abs_err {err:.3e} bound {bound:.1e} moved {moved:.4f} saturated {sat:.3f} "
         f"base_saturated {R.saturated_fraction(base):.3f}")
    assert moved > 1e-3, "the restatement does not move the image: the test would pass with the keyword ignored"
    assert sat <= 0.5, "the synthetic decoder saturates more than half of the pixels"
    assert err <= bound, (tag, mode, err, bound)


@pytest.mark.parametrize("mode", ["wavelet", "adain"])
@pytest.mark.parametrize("n_prompt,n_img,nipp,guidance", [(1, 1, 1, 5.0), (1, 1, 1, 1.0), (1, 1, 2, 5.0), (2, 1, 1, 5.0), (2, 2, 2, 5.0)],
                         ids=["cfg", "nocfg", "nipp2", "one_image_batch2", "two_images_nipp2"])
def test_pipeline_color_fix_equals_restatement_of_plain_call(penv, mode, n_prompt, n_img, nipp, guidance):
    cfg, pipe, lcm = penv
    kw = _call_kw(cfg, lcm, n_prompt, n_img, nipp, guidance)
    B = n_prompt * nipp
    base = pipe(output_type="pt", **kw).images.float().cpu()
    got = pipe(output_type="pt", color_fix=mode, **kw).images.float().cpu()
    assert got.shape == base.shape == (B, 3, 128, 128)
    _check_against_restatement(got, base, _reference_of(kw["image"], B, nipp), mode, f"n_prompt={n_prompt} n_img={n_img} nipp={nipp} g={guidance}")


def test_pipeline_none_and_omitted_are_bit_identical(penv):
    cfg, pipe, lcm = penv
    kw = _call_kw(cfg, lcm, 1, 1, 1, 5.0)
    a = pipe(output_type="pt", **kw).images
    b = pipe(output_type="pt", color_fix=None, **kw).images
    assert torch.equal(a, b)
    la = pipe(output_type="latent", **kw).images
    lb = pipe(output_type="latent", color_fix=None, **kw).images
    assert torch.equal(la, lb)


@pytest.mark.parametrize("mode", ["wavelet", "adain"])
def test_pipeline_pil_np_and_explicit_reference(penv, mode):
    import numpy as np
    cfg, pipe, lcm = penv
    kw = _call_kw(cfg, lcm, 1, 1, 1, 5.0)
    base = pipe(output_type="pt", **kw).images.float().cpu()
    want = R.apply(base.double(), _reference_of(kw["image"], 1, 1).double(), mode)
    pil = pipe(output_type="pil", color_fix=mode, **kw).images
    arr = np.asarray(pil[0]).astype(np.int64)
    want8 = (want[0].permute(1, 2, 0).numpy() * 255).round().astype(np.int64)
    assert arr.shape == (128, 128, 3) and np.abs(arr - want8).max() <= 1
    assert np.abs(arr - (base[0].permute(1, 2, 0).numpy() * 255).round()).mean() > 0.25          # and it is not the unfixed image
    npo = pipe(output_type="np", color_fix=mode, **kw).images
    assert npo.shape == (1, 128, 128, 3) and np.abs(npo[0] - want[0].permute(1, 2, 0).numpy()).max() <= 2e-5
    # an explicit reference (tensor, then the same as a PIL image) replaces the LQ pixels
    g = torch.Generator().manual_seed(77)
    ref8 = (torch.rand(1, 3, 128, 128, generator=g) * 255).round()
    ref = ref8 / 255.0
    got = pipe(output_type="pt", color_fix=mode, color_fix_reference=ref, **kw).images.float().cpu()
    _check_against_restatement(got, base, ref, mode, "explicit tensor reference")
    from PIL import Image
    im = Image.fromarray(ref8[0].permute(1, 2, 0).numpy().astype("uint8"))
    got_pil = pipe(output_type="pt", color_fix=mode, color_fix_reference=[im], **kw).images.float().cpu()
    assert torch.equal(got, got_pil)
    with pytest.raises(ValueError, match="128, 128"):
        pipe(output_type="pt", color_fix=mode, color_fix_reference=ref[:, :, :64, :64], **kw)


def test_pipeline_latent_image_needs_reference_and_preview_rows_stay_unfixed(penv):
    cfg, pipe, lcm = penv
    kw = _call_kw(cfg, lcm, 1, 1, 1, 5.0)
    lat = pipe.vae.encode_to_latent(kw["image"] * 2 - 1, eps=kw["vae_noise"]).cpu()
    kl = dict(kw, image=lat)
    with pytest.raises(ValueError, match="color_fix_reference"):
        pipe(output_type="pt", color_fix="wavelet", **kl)
    ref = _reference_of(kw["image"], 1, 1)
    base = pipe(output_type="pt", **kl).images.float().cpu()
    got = pipe(output_type="pt", color_fix="wavelet", color_fix_reference=ref, **kl).images.float().cpu()
    _check_against_restatement(got, base, ref, "wavelet", "latent image + reference")
    out0, rows0 = pipe(output_type="pt", return_dict=False, save_preview_row=True, **kw)
    out1, rows1 = pipe(output_type="pt", return_dict=False, save_preview_row=True, color_fix="adain", **kw)
    assert len(rows0) == len(rows1) > 0 and all(torch.equal(a, b) for a, b in zip(rows0, rows1))
    assert not torch.equal(out0, out1)


@pytest.mark.parametrize("mode", ["wavelet", "adain"])
def test_restore_single_step_color_fix(penv, mode):
    cfg, pipe, lcm = penv
    kw = _call_kw(cfg, lcm, 1, 1, 1, 1.0)
    args = dict(image=kw["image"], prompt_embeds=kw["prompt_embeds"], pooled_prompt_embeds=kw["pooled_prompt_embeds"],
                ip_adapter_image_embeds=kw["ip_adapter_image_embeds"], init_noise=kw["init_noise"], vae_noise=kw["vae_noise"])
    base = pipe.restore_single_step(output_type="pt", **args).images.float().cpu()
    same = pipe.restore_single_step(output_type="pt", color_fix=None, **args).images.float().cpu()
    got = pipe.restore_single_step(output_type="pt", color_fix=mode, **args).images.float().cpu()
    assert torch.equal(base, same)
    _check_against_restatement(got, base, _reference_of(kw["image"], 1, 1), mode, "restore_single_step")
    with pytest.raises(ValueError, match="latent"):
        pipe.restore_single_step(output_type="latent", color_fix=mode, **args)
    with pytest.raises(ValueError, match="None, 'wavelet' or 'adain'"):
        pipe.restore_single_step(output_type="pt", color_fix="lab", **args)


def test_tiled_decode_fix_applies_to_the_assembled_image(penv):
    """`vae.enable_tiling()` with a two-tile geometry (256-px tiles over a 256 x 320 image: latent
    32 x 40, stride 24, tiles at columns 0 and 24; every tile keeps the token counts the tiny nets' attention accepts): the
    correction sees the blended, assembled image, not the tiles."""
    cfg, pipe, lcm = penv
    g = torch.Generator().manual_seed(31)
    kw = _call_kw(cfg, lcm, 1, 1, 1, 5.0)
    kw.update(image=torch.rand(1, 3, 256, 320, generator=g), vae_noise=torch.randn(1, 4, 32, 40, generator=g),
              init_noise=torch.randn(1, 4, 32, 40, generator=g))
    vae = pipe.vae
    vae.tile_sample_size = 256
    try:
        plain = pipe(output_type="pt", **kw).images.float().cpu()
        vae.enable_tiling()
        base = pipe(output_type="pt", **kw).images.float().cpu()
        got = {m: pipe(output_type="pt", color_fix=m, **kw).images.float().cpu() for m in ("wavelet", "adain")}
    finally:
        vae.disable_tiling()
        vae.tile_sample_size = 1024
    assert base.shape == (1, 3, 256, 320) and not torch.equal(base, plain)      # the decode really was tiled
    for m in ("wavelet", "adain"):
        _check_against_restatement(got[m], base, _reference_of(kw["image"], 1, 1), m, "tiled decode")


def test_cli_color_fix_writes_what_its_python_twin_writes(tmp_path, dev):
    import numpy as np
    from PIL import Image
    import instantir_amd.infer as cli
    src, out = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    rng = np.random.default_rng(4)
    Image.fromarray(rng.integers(0, 255, (128, 128, 3), dtype=np.uint8)).save(src / "a.png")
    common = ["--test_path", str(src), "--synthetic", "tiny", "--num_inference_steps", "2", "--width", "128", "--height", "128",
              "--cfg", "5.0", "--seed", "5"]
    args = cli.build_parser().parse_args(common + ["--out_path", str(out), "--color_fix", "wavelet"])
    args0 = cli.build_parser().parse_args(common + ["--out_path", str(tmp_path / "out0")])
    orig = cli.resize_img
    cli.resize_img = lambda im, **kw: orig(im, max_side=128, min_side=128, **kw)
    try:
        torch.manual_seed(123)          # the VAE posterior sample draws from the global RNG
        cli.main(args, dev)
        torch.manual_seed(123)
        cli.main(args0, dev)
    finally:
        cli.resize_img = orig
    got = np.asarray(Image.open(out / "a.png"))
    unfixed = np.asarray(Image.open(tmp_path / "out0" / "a.png"))
    # the twin: the pipeline the CLI builds, called from Python with the keyword
    pipe, lcm = cli.build_pipeline(args, dev)
    cfg = pipe.cfg
    lq, _ = orig(Image.open(src / "a.png").convert("RGB"), max_side=128, min_side=128, width=128, height=128)
    g = torch.Generator().manual_seed(5)
    kw = dict(image=[lq], num_inference_steps=2, generator=torch.Generator(device=dev).manual_seed(5), guidance_scale=5.0,
              previewer_scheduler=lcm, preview_start=args.preview_start, control_guidance_end=args.creative_start,
              prompt_embeds=torch.randn(1, cfg.text_len, cfg.cross_attention_dim, generator=g),
              pooled_prompt_embeds=torch.randn(1, cfg.pooled_dim, generator=g),
              negative_prompt_embeds=torch.randn(1, cfg.text_len, cfg.cross_attention_dim, generator=g),
              negative_pooled_prompt_embeds=torch.randn(1, cfg.pooled_dim, generator=g),
              ip_adapter_image_embeds=[torch.randn(2, 1, cfg.resampler.seq_len, cfg.resampler.embedding_dim, generator=g)])
    torch.manual_seed(123)
    img = pipe(color_fix="wavelet", **kw).images[0]
    want = np.asarray(img.resize([128, 128], Image.BILINEAR))
    assert np.array_equal(got, want)
    assert not np.array_equal(got, unfixed)
