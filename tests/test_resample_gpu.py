"""GPU: device-side resampling (ops.resample / iir_resample_pass) against the fp64 restatement of the contract
(tests/resample_ref.py) and against PIL, its options, its determinism, and the encoder-preprocessing, pipeline and CLI wiring.

Bounds (set by the contract, not by what the kernel gives):
  float mode: |kernel - fp64 restatement| <= resample_ref.float_bound.  One pass sums n taps with fmaf from 0: n roundings,
      each at most 2^-24 of a partial sum bounded by L max|x| (L = the largest row sum of |w|, read from the tables); the fp32
      weights differ from the fp64 ones by 2^-24 relative, another 2^-24 L max|x|; one more unit covers second-order terms:
      e_pass = (taps + 2) 2^-24 L max|x|.  The vertical pass sees an input off by e_h and bounded by L_h max|x| + e_h, so
      e = L_v e_h + (taps_v + 2) 2^-24 L_v (L_h max|x| + e_h).
  quantised mode: never more than 1 LSB from the fp64 quantised restatement, on at most 0.5 % of the samples (round-off can
      flip a sample that sits on a rounding boundary; tests/test_resample_cpu.py confirms with the fp32-order restatement
      that these seeded inputs stay inside it); against PIL at most 1 LSB on at most 3 % (its 22-bit fixed-point weights).
  clamp / affine: the float bound scaled by max|scale|, plus 4 x 2^-24 of max|scale| max|v| + max|bias| (the two roundings of
      v * scale + bias and the fp32 rounding of the two vectors); the clamp is 1-Lipschitz.
Shapes: the smallest that can still go wrong -- one axis up and one down, both down, 1x1 sources and outputs, a 3-wide
output, widths that fill no wave evenly (more than one workgroup per plane), C = 1, 3, 4, N = 2, and one product-sized case.
Preprocessing features: PSNR of HipDinov2 features, device against host preprocessing, on a 2-layer 64-wide tower at 224 px;
first measurement 95.33 dB, bar 90.3 dB = that minus 5 dB (the encoder tests' bars sit at least that far under their figures)."""
import math

import numpy as np
import pytest
import torch

import resample_ref as R

pytestmark = pytest.mark.gpu

FLIP_CAP = 0.005
PIL_CAP = 0.03
CHANNELS = [3, 1, 4, 3, 1, 4, 3]                       # per geometry of R.GPU_GEOMETRIES
PREPROCESS_FEATURE_BAR = 90.3                          # dB: the first measurement, 95.33, minus 5 (module docstring)
_geo_id = lambda g: f"{g[0][0]}x{g[0][1]}-{g[1][0]}x{g[1][1]}"


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from instantir_amd import lib
    lib.load()
    return torch.device("cuda:0")


def _log(name, value):
    from conftest import record_psnr
    record_psnr("resample." + name, value)


def _sources(u8, dev, layout):
    """The same 8-bit image as the kernel's two source layouts: uint8 interleaved, or its values as fp32 planar."""
    if layout == "u8":
        return torch.from_numpy(u8).to(dev)
    return torch.from_numpy(R.planar(u8).astype(np.float32)).to(dev)


# ---- the kernel against the restatement -------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["u8", "f32"])
@pytest.mark.parametrize("gi", range(len(R.GPU_GEOMETRIES)), ids=[_geo_id(g) for g in R.GPU_GEOMETRIES])
def test_float_mode_matches_fp64_restatement(dev, gi, layout):
    from instantir_amd import ops
    (H, W), size = R.GPU_GEOMETRIES[gi]
    C = CHANNELS[gi]
    if layout == "u8":
        x = R.planar(R.noise_u8(31 + gi, 2, H, W, C)).astype(np.float64)
        src = torch.from_numpy(R.noise_u8(31 + gi, 2, H, W, C)).to(dev)
    else:
        x = np.random.default_rng(41 + gi).standard_normal((2, C, H, W)).astype(np.float32)
        src = torch.from_numpy(x).to(dev)
    for name in R.FILTERS:
        want = R.resize(x, size, name)
        bound = R.float_bound((H, W), size, name, float(np.abs(x).max()))
        got = ops.resample(src, size, name)
        torch.cuda.synchronize()
        err = np.abs(got.cpu().numpy().astype(np.float64) - want).max()
        print(f"float {layout} {name} 2x{C}x{H}x{W}->{size} max_abs_err {err:.3e} bound {bound:.3e}")
        _log(f"float_{layout}_{name}_{_geo_id(R.GPU_GEOMETRIES[gi])}.err_over_bound_1e-3", 1e3 * err / bound)
        assert got.shape == (2, C) + tuple(size) and got.dtype == torch.float32
        assert err <= bound, (name, err, bound)


@pytest.mark.parametrize("layout", ["u8", "f32"])
@pytest.mark.parametrize("gi", range(len(R.GPU_GEOMETRIES)), ids=[_geo_id(g) for g in R.GPU_GEOMETRIES])
def test_quantised_mode_matches_fp64_quantised_restatement(dev, gi, layout):
    from instantir_amd import ops
    (H, W), size = R.GPU_GEOMETRIES[gi]
    u8 = R.noise_u8(21, 2, H, W, 3)                        # the inputs test_resample_cpu.py rehearses
    src = _sources(u8, dev, layout)
    for name in R.FILTERS:
        want = R.resize(R.planar(u8), size, name, quantize=True)
        got = ops.resample(src, size, name, quantize=True).cpu().numpy()
        worst, frac = R.lsb_report(got, want)
        print(f"quantised {layout} {name} {H}x{W}->{size} max_diff {worst:.0f} differing {100 * frac:.3f} %")
        _log(f"quantised_{layout}_{name}_{_geo_id(R.GPU_GEOMETRIES[gi])}.differing_1e-6", 1e6 * frac)
        assert np.array_equal(got, np.round(got)) and got.min() >= 0 and got.max() <= 255
        assert worst <= 1 and frac <= FLIP_CAP, (name, worst, frac)


@pytest.mark.parametrize("name", R.FILTERS)
@pytest.mark.parametrize("geo", R.PIL_GEOMETRIES, ids=_geo_id)
def test_quantised_mode_against_pil(dev, name, geo):
    from instantir_amd import ops
    (H, W), size = geo
    u8 = R.noise_u8(5, 1, H, W, 3)
    got = ops.resample(torch.from_numpy(u8).to(dev), size, name, quantize=True)[0].permute(1, 2, 0).cpu().numpy()
    worst, frac = R.lsb_report(got, R.pil_resize(u8[0], size, name))
    print(f"pil {name} {H}x{W}->{size} max_diff {worst:.0f} differing {100 * frac:.2f} %")
    _log(f"pil_{name}_{_geo_id(geo)}.differing_1e-6", 1e6 * frac)
    assert worst <= 1 and frac <= PIL_CAP, (worst, frac)
    same = ops.resample(torch.from_numpy(u8).to(dev), (H, W), name, quantize=True)[0].permute(1, 2, 0).cpu().numpy()
    assert np.array_equal(same, u8[0])                      # equal sizes: exact, as PIL


# ---- options ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["u8", "f32"])
@pytest.mark.parametrize("size,window", [((129, 67), (5, 3, 100, 50)), ((257, 67), (250, 66, 7, 1)), ((129, 131), (0, 64, 129, 67)),
                                         ((300, 200), (1, 0, 298, 200)), ((257, 131), (100, 100, 3, 5))],
                         ids=["both", "horizontal_only", "vertical_only", "up", "same_size"])
def test_window_equals_the_same_window_of_the_full_result(dev, layout, size, window):
    from instantir_amd import ops
    src = _sources(R.noise_u8(8, 2, 257, 131, 3), dev, layout)
    y0, x0, h, w = window
    for name in R.FILTERS:
        for q in (False, True):
            full = ops.resample(src, size, name, quantize=q)
            part = ops.resample(src, size, name, quantize=q, window=window)
            assert part.shape == (2, 3, h, w) and part.is_contiguous()
            assert torch.equal(part, full[:, :, y0:y0 + h, x0:x0 + w]), (name, q)


@pytest.mark.parametrize("layout", ["u8", "f32"])
def test_affine_and_clamp(dev, layout):
    from instantir_amd import ops
    (H, W), size, C = (37, 53), (64, 40), 3
    u8 = R.noise_u8(9, 2, H, W, C)
    src = _sources(u8, dev, layout)
    x = R.planar(u8).astype(np.float64)
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    cases = [dict(scale=1 / 255.0), dict(scale=2 / 255.0, bias=-1.0), dict(clamp=(0.0, 255.0), scale=[1 / (255 * s) for s in std],
                                                                        bias=[-m / s for m, s in zip(mean, std)]),
             dict(clamp=(16.0, 235.0)), dict(bias=torch.tensor([1.0, 2.0, 3.0], device=dev)), dict(quantize=True, scale=1 / 255.0)]
    for name in R.FILTERS:
        fb = R.float_bound((H, W), size, name, 255.0)
        vmax = float(np.abs(R.resize(x, size, name)).max())
        for kw in cases:
            ref_kw = {k: (v.cpu().numpy() if torch.is_tensor(v) else ([v] * C if isinstance(v, float) else v)) for k, v in kw.items()}
            want = R.resize(x, size, name, **ref_kw)
            got = ops.resample(src, size, name, **kw).cpu().numpy().astype(np.float64)
            smax = float(np.abs(np.asarray(ref_kw.get("scale", [1.0]), dtype=np.float64)).max())
            bmax = float(np.abs(np.asarray(ref_kw.get("bias", [0.0]), dtype=np.float64)).max())
            bound = smax * fb + 4 * R.U * (smax * vmax + bmax)
            if kw.get("quantize"):
                # integers before the affine: compare them, then the affine alone
                worst, frac = R.lsb_report(np.round(got * 255.0), np.round(want * 255.0))
                assert worst <= 1 and frac <= FLIP_CAP
                q = ops.resample(src, size, name, quantize=True).cpu().numpy().astype(np.float64)
                assert np.abs(got - q * np.float32(1 / 255.0).astype(np.float64)).max() <= 4 * R.U
                continue
            err = np.abs(got - want).max()
            print(f"affine {layout} {name} {sorted(kw)} max_abs_err {err:.3e} bound {bound:.3e}")
            assert err <= bound, (name, kw, err, bound)
            if "clamp" in kw and "scale" not in kw:
                assert got.min() >= kw["clamp"][0] and got.max() <= kw["clamp"][1] and (got == kw["clamp"][0]).any()


def test_equal_sizes_without_options_are_a_bit_exact_copy(dev):
    from instantir_amd import ops
    x = torch.randn(2, 4, 37, 53, device=dev)
    x[0, 0, 0, 0] = float("inf")
    out = ops.resample(x, (37, 53), "lanczos")
    assert out.data_ptr() != x.data_ptr() and torch.equal(out, x)
    given = torch.empty_like(x)
    assert ops.resample(x, (37, 53), out=given) is given and torch.equal(given, x)
    u8 = R.noise_u8(10, 2, 37, 53, 3)
    out = ops.resample(torch.from_numpy(u8).to(dev), (37, 53), "bicubic")
    assert torch.equal(out.cpu(), torch.from_numpy(R.planar(u8)).float())


@pytest.mark.parametrize("geo,window", [(((37, 53), (64, 40)), None), (((96, 64), (37, 53)), (3, 5, 30, 40)), (((5, 7), (1, 1)), None),
                                        (((40, 64), (40, 100)), None), (((40, 64), (17, 64)), None), (((40, 64), (40, 64)), (1, 1, 38, 62))],
                         ids=["up_down", "down_window", "to_1x1", "horizontal_only", "vertical_only", "same_size_window"])
def test_out_of_buffer_reads_never_reach_the_output(dev, geo, window):
    """Source and destination are views into larger buffers: the source's surroundings hold NaN bit patterns, which an
    out-of-image read would carry into the output; the destination's surroundings hold a sentinel that must survive."""
    from instantir_amd import ops
    (H, W), size = geo
    h, w = (window[2], window[3]) if window else size
    n_src, n_dst, pad = 2 * 3 * H * W, 2 * 3 * h * w, 4096
    x = torch.from_numpy(R.planar(R.noise_u8(12, 2, H, W, 3)).astype(np.float32))
    sbuf = torch.full((n_src + 2 * pad,), float("nan"), device=dev)
    src = sbuf[pad:pad + n_src].view(2, 3, H, W)
    src.copy_(x)
    for name in R.FILTERS:
        for q in (False, True):
            dbuf = torch.full((n_dst + 2 * pad,), -7.0, device=dev)
            out = dbuf[pad:pad + n_dst].view(2, 3, h, w)
            ops.resample(src, size, name, quantize=q, window=window, out=out)
            torch.cuda.synchronize()
            assert torch.isfinite(out).all(), (name, q)
            assert (dbuf[:pad] == -7.0).all() and (dbuf[pad + n_dst:] == -7.0).all(), (name, q)
            assert torch.equal(out, ops.resample(x.to(dev), size, name, quantize=q, window=window))
    assert torch.isnan(sbuf[:pad]).all() and torch.isnan(sbuf[pad + n_src:]).all()


# ---- determinism -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geo", [((5, 7), (1, 1)), ((257, 131), (129, 67)), ((768, 1024), (1536, 2048))], ids=_geo_id)
def test_repeat_and_busy_neighbour_give_the_same_bits(dev, geo):
    from instantir_amd import ops
    (H, W), size = geo
    src = torch.from_numpy(R.noise_u8(13, 1, H, W, 3)).to(dev)
    keep = src.clone()
    first = {n: ops.resample(src, size, n, quantize=(n == "bicubic"), scale=1 / 255.0) for n in R.FILTERS}
    again = {n: ops.resample(src, size, n, quantize=(n == "bicubic"), scale=1 / 255.0) for n in R.FILTERS}
    torch.cuda.synchronize()
    assert all(torch.equal(first[n], again[n]) for n in R.FILTERS), "two runs differ"
    assert torch.equal(src, keep), "the source was modified"
    side = torch.cuda.Stream()
    a = torch.randn(2048, 2048, device=dev, dtype=torch.half)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(24):
            a = (a @ a).clamp_(-1, 1)
    busy = {n: ops.resample(src, size, n, quantize=(n == "bicubic"), scale=1 / 255.0) for n in R.FILTERS}
    torch.cuda.synchronize()
    assert all(torch.equal(first[n], busy[n]) for n in R.FILTERS), "a run beside a busy stream differs"


# ---- encoder preprocessing --------------------------------------------------------------------------------------------------
def _pil(seed, w, h):
    """A smooth seeded picture plus noise (full-range noise alone would make every encoder feature a noise feature)."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([127 + 100 * np.sin(xx / 9.0 + c) * np.cos(yy / 7.0 - c) for c in range(3)], axis=-1)
    return Image.fromarray(np.clip(base + rng.normal(0, 20, (h, w, 3)), 0, 255).astype(np.uint8))


@pytest.mark.parametrize("which", ["dinov2", "clip"])
@pytest.mark.parametrize("w,h", [(61, 47), (300, 200)])
def test_device_preprocess_is_within_one_lsb_of_the_host_form(dev, which, w, h):
    from instantir_amd import encoders as E
    pre = E.dinov2_preprocess if which == "dinov2" else E.clip_preprocess
    ims = [_pil(3, w, h), _pil(4, w, h)]
    raw = dict(mean=(0.0, 0.0, 0.0), std=(1 / 255.0,) * 3)           # pixels before normalisation, in 0..255 units
    host = np.round(pre(ims, **raw).numpy())
    got = pre(ims, device=dev, **raw)
    assert got.is_cuda and got.dtype == torch.float32 and got.shape == (2, 3, 224, 224)
    worst, frac = R.lsb_report(np.round(got.cpu().numpy()), host)
    print(f"preprocess {which} {w}x{h} max_diff {worst:.0f} differing {100 * frac:.2f} %")
    _log(f"preprocess_{which}_{w}x{h}.differing_1e-6", 1e6 * frac)
    assert worst <= 1 and frac <= PIL_CAP
    # normalised: the affine is v / (255 std) - mean / std; a tensor of 0..255-valued pixels is the same raw image
    want, dv = pre(ims), pre(ims, device=dev)
    assert (dv.cpu() - want).abs().max().item() <= 1.001 / (255 * 0.224)
    t = torch.from_numpy(np.stack([np.asarray(im) for im in ims])).to(dev)
    assert torch.equal(pre(t, device=dev), dv) and torch.equal(pre(t.permute(0, 3, 1, 2).float().contiguous(), device=dev), dv)
    assert torch.equal(pre([ims[0], _pil(5, w + 3, h)], device=dev)[:1], dv[:1])     # mixed sizes: one launch pair per size


def test_device_preprocess_features_on_the_tiny_tower(dev):
    from PIL import Image
    from test_encoders_gpu import _model
    from instantir_amd import encoders as E
    from instantir_amd.pipeline import InstantIRPipeline
    _, sd = _model(64, 1, 2, 224, 8)
    enc = E.HipDinov2(sd, dev)
    ims = [_pil(3, 300, 200), _pil(4, 300, 200)]
    want = enc(E.dinov2_preprocess(ims)).float().cpu()
    got = enc(E.dinov2_preprocess(ims, device=dev)).float().cpu()
    p = 10 * math.log10(want.abs().max().item() ** 2 / max(((got - want) ** 2).mean().item(), 1e-30))
    print(f"preprocess features PSNR {p:.2f} dB bar {PREPROCESS_FEATURE_BAR}")
    _log("preprocess_features_psnr", p)
    assert torch.isfinite(got).all() and got.shape == want.shape == (2, 257, 64)
    assert p >= PREPROCESS_FEATURE_BAR, p
    # the pipeline's switch: off by default, and encode_image follows it
    pipe = InstantIRPipeline.__new__(InstantIRPipeline)
    pipe.device, pipe.image_encoder, pipe._device_preprocess = dev, enc, False
    f_host, _ = pipe.encode_image(ims)
    pipe.enable_device_preprocess()
    f_dev, _ = pipe.encode_image(ims)
    pipe.disable_device_preprocess()
    f_off, _ = pipe.encode_image(ims)
    assert torch.equal(f_host.float().cpu(), want) and torch.equal(f_dev.float().cpu(), got) and torch.equal(f_off, f_host)
    # the default `ip_adapter_image` of a call with work_size: the working image as its 8-bit PIL copy would be preprocessed
    work = _work_image(ims, dev, "bilinear")
    copies = [Image.fromarray(a) for a in (work * 255).round().permute(0, 2, 3, 1).to(torch.uint8).cpu().numpy()]
    px = pipe._preprocess_work_image(work)
    assert torch.equal(px, E.dinov2_preprocess(copies, device=dev))
    assert torch.equal(pipe.encode_image(px)[0], enc(px))                   # and encode_image takes it as it stands


# ---- pipeline ----------------------------------------------------------------------------------------------------------------------
WORK, OUT = (128, 128), (90, 150)


@pytest.fixture(scope="module")
def penv(dev):
    """The tiny-loop fixture of tests/loop_ref.py (B = 2, latent 16 x 16) with the tiny VAE attached: one loop geometry."""
    import loop_ref
    from instantir_amd import weights as W
    from instantir_amd.config import VAEConfig
    from instantir_amd.schedulers import LCMSingleStepScheduler
    from instantir_amd.vae import HipVAE
    env = loop_ref.tiny_env()
    pipe = loop_ref.pipe(env)
    vc = VAEConfig.tiny()
    pipe.vae = HipVAE(vc, W.synth_state_dict(W.vae_decoder_specs(vc) + W.vae_encoder_specs(vc), 21, dtype=torch.bfloat16), dev)
    inp = env[4]
    g = torch.Generator().manual_seed(5)
    kw = dict(prompt_embeds=inp["pe"], pooled_prompt_embeds=inp["pooled"], negative_prompt_embeds=inp["npe"],
              negative_pooled_prompt_embeds=inp["npooled"], ip_adapter_image_embeds=[inp["img"]], init_noise=inp["init_noise"],
              vae_noise=torch.randn(2, 4, 16, 16, generator=g), num_inference_steps=2, guidance_scale=7.0,
              previewer_scheduler=LCMSingleStepScheduler.from_config(pipe.scheduler.config))
    pils = [_pil(6, 75, 50), _pil(7, 75, 50)]
    yield pipe, kw, pils
    assert pipe._device_preprocess is False and pipe.vae.use_tiling is False


def _work_image(pils, dev, name):
    from instantir_amd import ops
    u8 = torch.from_numpy(np.stack([np.asarray(im) for im in pils])).to(dev)
    return ops.resample(u8, WORK, name, quantize=True, scale=1 / 255.0)


@pytest.mark.parametrize("name", ["bilinear", "lanczos"])
def test_pipeline_resize_equals_plain_call_between_two_resamples(penv, dev, name):
    from instantir_amd import ops
    pipe, kw, pils = penv
    # PIL input: quantised mode in, float mode out
    got = pipe(image=pils, work_size=WORK, output_size=OUT, resample=name, output_type="pt", **kw).images
    plain = pipe(image=_work_image(pils, dev, name), output_type="pt", **kw).images
    assert plain.shape == (2, 3) + WORK and got.shape == (2, 3) + OUT
    assert torch.equal(got, ops.resample(plain.contiguous(), OUT, name, clamp=(0.0, 1.0)))
    # a float tensor input: float mode with a clamp to [0, 1] on both sides
    t = torch.rand(2, 3, 50, 75, generator=torch.Generator().manual_seed(8))
    got_t = pipe(image=t, work_size=WORK, output_size=OUT, resample=name, output_type="pt", **kw).images
    plain_t = pipe(image=ops.resample(t.to(dev), WORK, name, clamp=(0.0, 1.0)), output_type="pt", **kw).images
    assert torch.equal(got_t, ops.resample(plain_t.contiguous(), OUT, name, clamp=(0.0, 1.0)))
    assert not torch.equal(got_t, got)
    # each argument alone
    only_in = pipe(image=pils, work_size=WORK, resample=name, output_type="pt", **kw).images
    assert torch.equal(only_in, plain)
    only_out = pipe(image=_work_image(pils, dev, name), output_size=OUT, resample=name, output_type="np", **kw).images
    assert only_out.shape == (2,) + OUT + (3,) and np.array_equal(only_out, got.permute(0, 2, 3, 1).cpu().numpy())


def test_pipeline_omitted_arguments_give_todays_bits(penv, dev):
    pipe, kw, pils = penv
    img = _work_image(pils, dev, "bilinear")
    for ot in ("pt", "latent"):
        a = pipe(image=img, output_type=ot, **kw).images
        b = pipe(image=img, output_type=ot, work_size=None, output_size=None, resample="bilinear", **kw).images
        assert torch.equal(a, b)


def test_pipeline_color_fix_uses_the_work_size_image(penv, dev):
    pipe, kw, pils = penv
    got = pipe(image=pils, work_size=WORK, resample="bicubic", color_fix="wavelet", output_type="pt", **kw).images
    want = pipe(image=_work_image(pils, dev, "bicubic"), color_fix="wavelet", output_type="pt", **kw).images
    unfixed = pipe(image=pils, work_size=WORK, resample="bicubic", output_type="pt", **kw).images
    assert torch.equal(got, want) and not torch.equal(got, unfixed)


def test_pipeline_pil_output_is_within_one_lsb_of_pils_resize(penv, dev):
    from PIL import Image
    pipe, kw, pils = penv
    img = _work_image(pils, dev, "bilinear")
    for name, flt in (("bilinear", Image.BILINEAR), ("bicubic", Image.BICUBIC)):
        got = pipe(image=img, output_size=OUT, resample=name, output_type="pil", **kw).images
        plain = pipe(image=img, output_type="pil", **kw).images
        assert len(got) == 2 and got[0].size == (OUT[1], OUT[0])
        for a, b in zip(got, plain):
            worst, frac = R.lsb_report(np.asarray(a), np.asarray(b.resize((OUT[1], OUT[0]), flt)))
            print(f"pipeline pil {name} max_diff {worst:.0f} differing {100 * frac:.2f} %")
            assert worst <= 1 and frac <= PIL_CAP
    out, rows = pipe(image=img, output_size=OUT, output_type="pt", return_dict=False, save_preview_row=True, **kw)
    assert out.shape[2:] == OUT and len(rows) > 0 and all(r.shape[2:] == WORK for r in rows)     # the preview row is never resampled


def test_pipeline_refusals(penv, dev):
    pipe, kw, pils = penv
    lat = torch.randn(2, 4, 16, 16)
    with pytest.raises(ValueError, match="LQ latent"):
        pipe(image=lat, work_size=WORK, output_type="latent", **kw)
    with pytest.raises(ValueError, match="output_type='latent'"):
        pipe(image=pils, work_size=WORK, output_size=OUT, output_type="latent", **kw)
    with pytest.raises(ValueError, match="resample must be one of"):
        pipe(image=pils, work_size=WORK, resample="nearest", **kw)
    with pytest.raises(ValueError, match="needs work_size or output_size"):
        pipe(image=lat, resample="lanczos", output_type="latent", **kw)
    with pytest.raises(ValueError, match="multiple of 8"):
        pipe(image=pils, work_size=(128, 100), **kw)
    with pytest.raises(ValueError, match="multiple of 8"):                        # without work_size the library still resizes nothing
        pipe(image=pils, **kw)
    with pytest.raises(ValueError, match="negative values"):
        pipe(image=torch.rand(2, 3, 50, 75) - 0.5, work_size=WORK, **kw)
    with pytest.raises(ValueError, match="128, 128"):                            # restore_map sizes refer to the working size
        pipe(image=pils, work_size=WORK, restore_map=torch.ones(50, 75), output_type="pt", **kw)
    m = torch.ones(128, 128)
    m[:64] = 0
    kept = pipe(image=pils, work_size=WORK, restore_map=m, map_feather=0, output_type="pt", **kw).images
    # the composite's original is the working image w, as the pipeline maps it to [-1, 1] and back: (2 w - 1) / 2 + 0.5 rounds
    # once at magnitude <= 1 and once at <= 1, so it is w to 2^-23
    assert (kept[:, :, :60] - _work_image(pils, dev, "bilinear")[:, :, :60]).abs().max().item() <= 2.0 ** -23


def test_cli_device_resize_writes_what_its_python_twin_writes(tmp_path, dev):
    import instantir_amd.infer as cli
    src, out = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    _pil(9, 100, 76).save(src / "a.png")
    common = ["--test_path", str(src), "--synthetic", "tiny", "--num_inference_steps", "2", "--width", "96", "--height", "96",
              "--cfg", "5.0", "--seed", "5"]
    args = cli.build_parser().parse_args(common + ["--out_path", str(out), "--device_resize", "--resample", "bicubic"])
    orig = cli.resize_plan
    cli.resize_plan = lambda size, **kw: orig(size, max_side=128, min_side=128, **kw)
    try:
        assert cli.resize_plan((100, 76), width=96, height=96) == ((128, 128), (96, 96))
        torch.manual_seed(123)          # the VAE posterior sample draws from the global RNG
        cli.main(args, dev)
    finally:
        cli.resize_plan = orig
    from PIL import Image
    got = np.asarray(Image.open(out / "a.png"))
    pipe, lcm = cli.build_pipeline(args, dev)
    cfg = pipe.cfg
    g = torch.Generator().manual_seed(5)
    kw = dict(image=[Image.open(src / "a.png").convert("RGB")], num_inference_steps=2, generator=torch.Generator(device=dev).manual_seed(5),
              guidance_scale=5.0, previewer_scheduler=lcm, preview_start=args.preview_start, control_guidance_end=args.creative_start,
              prompt_embeds=torch.randn(1, cfg.text_len, cfg.cross_attention_dim, generator=g),
              pooled_prompt_embeds=torch.randn(1, cfg.pooled_dim, generator=g),
              negative_prompt_embeds=torch.randn(1, cfg.text_len, cfg.cross_attention_dim, generator=g),
              negative_pooled_prompt_embeds=torch.randn(1, cfg.pooled_dim, generator=g),
              ip_adapter_image_embeds=[torch.randn(2, 1, cfg.resampler.seq_len, cfg.resampler.embedding_dim, generator=g)])
    torch.manual_seed(123)
    want = np.asarray(pipe(work_size=(128, 128), output_size=(96, 96), resample="bicubic", **kw).images[0])
    assert got.shape == (96, 96, 3) and np.array_equal(got, want)
