"""CPU: the host side of synthetic degradation (instantir_amd.degrade: kernel builders, recipes), the restatements of
tests/degrade_ref.py against known answers, statistics, an independent JPEG implementation and each other, and every refusal
of the three entries, their wrappers and the CLI flags that needs no GPU."""
import ctypes
import io
import math

import numpy as np
import pytest
import torch

import degrade_ref as R
from instantir_amd import degrade as D


# ---- kernel builders --------------------------------------------------------------------------------------------------------
def test_kernels_sum_to_one_and_are_symmetric():
    for k in (D.gaussian_kernel(21, 2.0), D.generalized_gaussian_kernel(13, 1.5, 0.7), D.plateau_kernel(9, 1.2, 1.8),
              D.sinc_kernel(21, 1.3), D.sinc_kernel(7, math.pi)):
        assert k.dtype == np.float64 and abs(k.sum() - 1.0) < 1e-14
        assert np.array_equal(k, k.T) and np.array_equal(k, k[::-1]) and np.array_equal(k, k[:, ::-1])       # the isotropic ones
    for k in (D.gaussian_kernel(15, 2.5, 0.8, 0.6), D.generalized_gaussian_kernel(15, 2.5, 1.4, 0.8, -1.0), D.plateau_kernel(11, 2.0, 1.5, 0.7, 2.0)):
        assert abs(k.sum() - 1.0) < 1e-14
        assert np.allclose(k, k[::-1, ::-1], rtol=0, atol=1e-17) and not np.allclose(k, k.T)                # a point symmetry alone
    # rotating by 90 degrees swaps the axes
    assert np.allclose(D.gaussian_kernel(9, 2.0, 0.5, math.pi / 2), D.gaussian_kernel(9, 0.5, 2.0, 0.0), rtol=0, atol=1e-15)


def test_isotropic_gaussian_against_its_closed_form():
    k, s = 11, 1.7
    g = np.exp(-0.5 * (np.arange(k) - k // 2) ** 2 / s ** 2)
    want = np.outer(g, g) / np.outer(g, g).sum()
    assert np.abs(D.gaussian_kernel(k, s) - want).max() < 1e-15
    assert np.abs(D.generalized_gaussian_kernel(k, s, 1.0) - want).max() < 1e-15                             # beta 1: the Gaussian


def test_bessel_j1_and_the_sinc_kernel_against_scipy():
    from scipy.special import j1
    x = np.linspace(0.0, 64.0, 4097)
    assert np.abs(D.bessel_j1(x) - j1(x)).max() < 1e-13
    for ksize, wc in ((21, math.pi / 5), (21, math.pi), (7, 2.0)):
        r = ksize // 2
        yy, xx = np.mgrid[-r:r + 1, -r:r + 1]
        rho = np.hypot(xx, yy)
        want = np.where(rho > 0, wc * j1(wc * rho) / (2 * np.pi * np.where(rho > 0, rho, 1)), wc * wc / (4 * np.pi))
        assert np.abs(D.sinc_kernel(ksize, wc) - want / want.sum()).max() < 1e-13


def test_pad_kernel():
    k = D.gaussian_kernel(7, 1.0)
    p = D.pad_kernel(k, 21)
    assert p.shape == (21, 21) and np.array_equal(p[7:14, 7:14], k) and p.sum() == k.sum() and np.count_nonzero(p) == 49
    assert D.pad_kernel(k, 7) is not k and np.array_equal(D.pad_kernel(k, 7), k)
    for bad in (np.ones((3, 5)), np.ones((4, 4)), np.ones((23, 23))):
        with pytest.raises(ValueError):
            D.pad_kernel(bad, 21)


# ---- recipes ----------------------------------------------------------------------------------------------------------------
def test_sample_recipe_is_a_pure_function_of_preset_seed_and_name():
    a = D.sample_recipe("realesrgan", 7, "a.png")
    assert a == D.sample_recipe("realesrgan", 7, "a.png") and a.to_json() == D.sample_recipe("realesrgan", 7, "a.png").to_json()
    assert a != D.sample_recipe("realesrgan", 8, "a.png") and a != D.sample_recipe("realesrgan", 7, "b.png")
    b = D.sample_recipe("bicubic", 7, "a.png")
    assert b == D.sample_recipe("bicubic", 0, "zzz") and len(b.stages) == 1 and b.stages[0].scale == 0.25 and b.sf == 4 and b.resize_lq
    assert b.stages[0].blur is None and b.stages[0].noise_sigma == 0 and b.stages[0].jpeg_quality == 0 and b.final_sinc is None
    assert D.sample_recipe("bicubic", 0, sf=2, resize_lq=False).stages[0].scale == 0.5
    with pytest.raises(ValueError, match="preset"):
        D.sample_recipe("esrgan", 0)
    assert D.noise_seed(7, "a.png") == D.noise_seed(7, "a.png") != D.noise_seed(7, "b.png") and 0 <= D.noise_seed(2 ** 64 - 1, "x") < 2 ** 64


def test_every_drawn_value_stays_inside_its_range():
    """2000 seeds of the realesrgan preset against the table of utils/degradation_pipeline.py:20-64"""
    opt = D.REALESRGAN
    seen = {"blur_none": 0, "sinc_none": 0, "jpeg_first": 0, "gray": 0, "up": 0, "down": 0, "keep": 0}
    for seed in range(2000):
        r = D.sample_recipe("realesrgan", seed, "f.png")
        assert len(r.stages) == 2 and r.sf == 4 and r.resize_lq and r.final_filter in ("bilinear", "bicubic")
        for i, s in enumerate(r.stages):
            if s.blur is None:
                assert i == 1
                seen["blur_none"] += 1
            else:
                assert s.blur.shape[0] == s.blur.shape[1] and s.blur.shape[0] in D.KERNEL_SIZES and abs(s.blur.sum() - 1) < 1e-12
            lo, hi = opt["resize_range"][i]
            rel = s.scale * (1 if i == 0 else r.sf)
            assert lo <= rel <= hi and s.resize_filter in ("bilinear", "bicubic")
            seen["up" if rel > 1 else "down" if rel < 1 else "keep"] += 1
            assert opt["noise_range"][i][0] <= s.noise_sigma <= opt["noise_range"][i][1]
            assert opt["jpeg_range"][i][0] <= s.jpeg_quality <= opt["jpeg_range"][i][1]
            seen["gray"] += s.gray_noise
        if r.final_sinc is None:
            seen["sinc_none"] += 1
        else:
            assert r.final_sinc.shape[0] in D.KERNEL_SIZES and abs(r.final_sinc.sum() - 1) < 1e-12
        seen["jpeg_first"] += r.jpeg_before_final_resize
    # the probabilities, within 5 sigma of a binomial
    for key, n, p in (("blur_none", 2000, 0.2), ("sinc_none", 2000, 0.2), ("jpeg_first", 2000, 0.5), ("gray", 4000, 0.4),
                      ("up", 4000, 0.25), ("down", 4000, 0.55), ("keep", 4000, 0.2)):
        assert abs(seen[key] - n * p) <= 5 * math.sqrt(n * p * (1 - p)), (key, seen[key])


def test_recipe_json_round_trip_is_exact():
    for r in (D.sample_recipe("realesrgan", 3, "x"), D.sample_recipe("bicubic", 0), D.Recipe([], final_sinc=D.sinc_kernel(9, 1.0), sf=2, resize_lq=False)):
        back = D.Recipe.from_json(r.to_json())
        assert back.to_json() == r.to_json() and back.sf == r.sf and back.resize_lq == r.resize_lq
        for a, b in zip(r.stages, back.stages):
            assert (a.blur is None) == (b.blur is None) and (a.blur is None or a.blur.tobytes() == b.blur.tobytes())
            assert (a.scale, a.resize_filter, a.noise_sigma, a.gray_noise, a.jpeg_quality) == (b.scale, b.resize_filter, b.noise_sigma, b.gray_noise, b.jpeg_quality)
        assert (r.final_sinc is None) == (back.final_sinc is None) and (r.final_sinc is None or r.final_sinc.tobytes() == back.final_sinc.tobytes())
    for bad in ("[1, 2]", "{\"sf\": 4}", "not json"):
        with pytest.raises(ValueError):
            D.Recipe.from_json(bad)
    for kw in (dict(scale=0.0), dict(resize_filter="area"), dict(noise_sigma=300.0), dict(jpeg_quality=100.0), dict(blur=np.ones((4, 4)))):
        with pytest.raises(ValueError):
            D.Stage(**kw)


# ---- the generator and the normal transform ---------------------------------------------------------------------------------
def test_philox_known_answers():
    for counter, key, want in R.PHILOX_KNOWN:
        got = R.philox4x32_10([np.uint32(c) for c in counter], key)
        assert tuple(int(v) for v in got) == want


def test_uniforms_are_the_contracts_fp32_values():
    r = np.array([0, 255, 256, (1 << 31) - 1, 1 << 31, (1 << 31) + 256, (1 << 32) - 1], np.uint32)
    u = R.uniforms32(r)
    assert u.dtype == np.float32 and u[0] == u[1] == np.float32(2.0 ** -25) and u[2] == np.float32(1.5 * 2.0 ** -24)
    assert u[3] == np.float32((2 ** 23 - 0.5) * 2.0 ** -24)                  # exact below 2^23
    assert u[4] == np.float32(0.5) and u[5] == np.float32((2 ** 23 + 2) * 2.0 ** -24) and u[6] == np.float32(1.0)   # ties to even above
    assert (u > 0).all() and (u <= 1).all()


def test_normal_transform_statistics():
    """2^18 samples of the fp64 restatement: mean, variance, lag-1 correlation along x and across channels"""
    z = R.normal64((1, 4, 256, 256), seed=0x1234567890abcdef, stream=2)
    n = z.size
    assert n == 1 << 18 and np.isfinite(z).all() and np.abs(z).max() <= R.Z_MAX
    assert abs(z.mean()) <= 5 / math.sqrt(n)
    assert abs(z.var() - 1.0) <= 5 * math.sqrt(2.0 / n)
    assert abs((z[..., 1:] * z[..., :-1]).mean()) <= 5 / math.sqrt(n)
    assert abs((z[:, 1:] * z[:, :-1]).mean()) <= 5 / math.sqrt(n)
    g = R.normal64((1, 3, 8, 8), seed=5, gray=True)
    assert np.array_equal(g[:, 0], g[:, 1]) and np.array_equal(g[:, 0], g[:, 2])
    assert not np.array_equal(R.normal64((1, 3, 8, 8), 5, 0), R.normal64((1, 3, 8, 8), 5, 1))


# ---- the JPEG restatement against libjpeg -----------------------------------------------------------------------------------
def _psnr(a, b):
    return 10 * math.log10(255.0 ** 2 / np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2))


@pytest.mark.parametrize("q", [30, 50, 75, 95])
def test_jpeg_restatement_against_pil(q):
    """The fp64 round trip against PIL's libjpeg round trip (4:2:0) of a seeded smooth-plus-noise 48 x 48 image.  libjpeg rounds
    its tables to integers and upsamples chroma with a triangle filter, so this is a sanity bar: the two must stand at least
    3 dB closer to each other than either stands to the uncompressed input.  Measured (between; ours, PIL's against the input):
    q 30: 42.06; 32.44, 32.56.  q 50: 46.25; 33.85, 33.89.  q 75: 44.66; 35.16, 35.26.  q 95: 44.65; 36.62, 36.58 dB."""
    from PIL import Image
    img = R.smooth_noise_image((1, 3, 48, 48), 1)
    ours = R.jpeg64(img.astype(np.float32) / np.float32(255.0), [q])["out"][0] * 255.0
    buf = io.BytesIO()
    Image.fromarray(img[0].transpose(1, 2, 0)).save(buf, format="JPEG", quality=q, subsampling=2)
    pil = np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB")).transpose(2, 0, 1)
    between, a, b = _psnr(ours, pil), _psnr(ours, img[0]), _psnr(pil, img[0])
    print(f"q {q}: between {between:.2f} dB; ours {a:.2f} dB, PIL's {b:.2f} dB against the input")
    assert between >= max(a, b) + 3.0


# ---- fp32 restatements inside the derived bounds --------------------------------------------------------------------------------
def test_filter2d_restatements_agree():
    g = np.random.default_rng(0)
    for shape, k in (((2, 3, 11, 13), 21), ((1, 3, 37, 67), 7), ((1, 1, 32, 32), 1)):
        x = g.random(shape, dtype=np.float32)
        t = g.random((shape[0], k, k)) - 0.2
        t = (t / t.sum(axis=(1, 2), keepdims=True)).astype(np.float32)
        assert (np.abs(R.filter2d32(x, t) - R.filter2d64(x, t)) <= R.filter2d_bound(x, t)).all()
    x = g.random((1, 2, 5, 6), dtype=np.float32)
    pulse = np.zeros((1, 3, 3), np.float32)
    pulse[0, 0, 2] = 1.0                                                   # out[y][x] = in[refl(y - 1)][refl(x + 1)]
    want = x[:, :, [1, 0, 1, 2, 3]][:, :, :, [1, 2, 3, 4, 5, 4]]
    assert np.array_equal(R.filter2d64(x, pulse), want) and np.array_equal(R.filter2d32(x, pulse), want)


def test_noise_restatements_agree():
    x = np.random.default_rng(1).random((2, 3, 19, 23), dtype=np.float32)
    sig = np.array([0.0, 50.0], np.float32)
    want, _ = R.noise64(x, sig, 9, 1)
    got = R.noise32(x, sig, 9, 1)
    assert got.dtype == np.float32 and (np.abs(got - want) <= R.noise_bound(x, sig, R.NOISE_Z_ULPS)).all()
    assert got[0].tobytes() == x[0].tobytes()


@pytest.mark.parametrize("q", [30.0, 49.5, 50.0, 95.0])
def test_jpeg_restatements_agree(q):
    x = R.exact_jpeg_input((2, 3, 32, 48), (q, q), seed=5)
    res = R.jpeg64(x, (q, q))
    assert res["tie_y"].min() > 0.1 and res["tie_c"].min() > 0.1 and 0.05 <= x.min() and x.max() <= 0.95
    assert (np.abs(R.jpeg32(x, (q, q)) - res["out"]) <= res["err"]).all()
    y = R.smooth_noise_image((1, 3, 17, 33), 3).astype(np.float32) / np.float32(255.0)
    res = R.jpeg64(y, [q])
    keep, share = R.jpeg_keep_mask(res, 17, 33)
    kept = np.broadcast_to(keep[:, None], y.shape)
    assert share.max() <= 0.10 and (np.abs(R.jpeg32(y, [q]) - res["out"])[kept] <= res["err"][kept]).all()


def test_jpeg_restatement_properties():
    flat = np.full((1, 3, 16, 16), 0.5, np.float32)
    assert np.abs(R.jpeg64(flat, [75])["out"] - 0.5).max() < 1.5 / 255            # a flat image keeps its level to within a DC step
    assert R.quality_factor(49.5) == 5000 / 49.5 / 100 and R.quality_factor(50) == 1.0 and R.quality_factor(95) == pytest.approx(0.1)
    assert R.T_LUMA[0, 1] == 11 and R.T_LUMA[1, 0] == 12 and R.T_CHROMA[0, 3] == 47 and R.T_LUMA[7, 7] == 99
    assert np.allclose(R.DCT @ R.DCT.T, np.eye(8), atol=1e-15)


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_entries_refuse_bad_arguments_without_a_gpu():
    """IIR_EINVAL before any HIP call; every call below is invalid, so none of them launches."""
    from instantir_amd import lib
    h = lib.load()
    P, Q = 1 << 20, 1 << 28
    f = lambda in_=P, taps=P, N=1, C=3, H=32, W=32, k=21, out=Q: h.iir_filter2d_f32(in_, taps, N, C, H, W, k, out, None)
    assert f(in_=None) == -1 and f(taps=None) == -1 and f(out=None) == -1
    assert f(N=0) == -1 and f(C=0) == -1 and f(H=0) == -1 and f(W=-1) == -1 and f(H=32769) == -1 and f(N=21846) == -1
    assert f(k=0) == -1 and f(k=8) == -1 and f(k=23) == -1 and f(k=-3) == -1
    assert f(H=10) == -1 and f(W=10) == -1 and f(k=7, H=3) == -1                                  # H, W > r
    assert f(out=P) == -1 and f(out=P + 4) == -1 and f(out=P - 4) == -1                           # neighbours are read
    n = lambda in_=P, sigma=P, N=1, C=3, H=32, W=32, out=Q: h.iir_add_gaussian_noise_f32(in_, sigma, N, C, H, W, 1, 0, 0, out, None)
    assert n(in_=None) == -1 and n(sigma=None) == -1 and n(out=None) == -1
    assert n(N=0) == -1 and n(C=-1) == -1 and n(H=0) == -1 and n(W=0) == -1
    assert n(H=65536, W=65536) == -1 and n(N=8192, C=64, H=32768, W=32768) == -1                  # H W < 2^32; the grid
    assert n(out=P + 4) == -1
    j = lambda in_=P, q=P, N=1, C=3, H=32, W=32, out=Q: h.iir_jpeg_roundtrip_f32(in_, q, N, C, H, W, out, None)
    assert j(in_=None) == -1 and j(q=None) == -1 and j(out=None) == -1
    assert j(C=1) == -1 and j(C=4) == -1 and j(N=0) == -1 and j(N=65536) == -1 and j(H=0) == -1 and j(W=32769) == -1
    assert j(out=P + 4) == -1
    assert h.iir_abi_version() == 3


def test_wrappers_refuse_bad_arguments_without_a_gpu():
    from instantir_amd import ops
    x = torch.zeros(2, 3, 16, 16)
    t = torch.ones(2, 3, 3) / 9
    for bad in (dict(x=x.double()), dict(x=x[0]), dict(x=x[:, :, ::2]), dict(taps=t.double()), dict(taps=torch.ones(2, 4, 4)),
                dict(taps=torch.ones(3, 3, 3)), dict(taps=torch.ones(2, 3, 5)), dict(taps=torch.ones(2, 23, 23)), dict(taps=torch.ones(2, 21, 21), x=torch.zeros(2, 3, 10, 16)),
                dict(out=x), dict(out=torch.zeros(2, 3, 16, 8)), dict(out=torch.zeros(2, 3, 16, 16, dtype=torch.float64))):
        a = dict(x=x, taps=t)
        a.update(bad)
        with pytest.raises(ValueError, match="filter2d"):
            ops.filter2d(**a)
    with pytest.raises(ValueError, match="no host path"):
        ops.filter2d(x, t)                                                 # valid but for the device
    for bad in (dict(sigma=-1.0), dict(sigma=256.0), dict(sigma=[1.0, 2.0, 3.0]), dict(sigma=float("nan")), dict(sigma="x"), dict(seed=-1),
                dict(seed=1 << 64), dict(seed=1.5), dict(stream=1 << 32), dict(stream=-1), dict(x=x.half()), dict(out=torch.zeros(2, 3, 8, 8))):
        a = dict(x=x, sigma=5.0, seed=1)
        a.update(bad)
        with pytest.raises(ValueError, match="add_gaussian_noise"):
            ops.add_gaussian_noise(**a)
    with pytest.raises(ValueError, match="no host path"):
        ops.add_gaussian_noise(x, [0.0, 255.0], (1 << 64) - 1, stream=(1 << 32) - 1, out=x)
    for bad in (dict(quality=0.5), dict(quality=99.5), dict(quality=[50.0]), dict(quality=torch.tensor([50.0, 100.0])), dict(x=torch.zeros(2, 1, 16, 16)),
                dict(x=torch.zeros(2, 4, 16, 16)), dict(out=torch.zeros(2, 3, 16, 16)[:, :, :8])):
        a = dict(x=x, quality=75.0)
        a.update(bad)
        with pytest.raises(ValueError, match="jpeg_roundtrip"):
            ops.jpeg_roundtrip(**a)
    with pytest.raises(ValueError, match="no host path"):
        ops.jpeg_roundtrip(x, torch.tensor([1.0, 99.0]), out=x)
    big = torch.zeros(2 * 3 * 16 * 16 + 8)
    shifted = big[8:].view(2, 3, 16, 16)
    for fn, kw in ((ops.add_gaussian_noise, dict(sigma=1.0, seed=0)), (ops.jpeg_roundtrip, dict(quality=50.0))):
        with pytest.raises(ValueError, match="overlaps"):
            fn(big[:-8].view(2, 3, 16, 16), out=shifted, **kw)


def test_cli_flag_refusals(tmp_path):
    import instantir_amd.infer as cli
    parse = lambda *extra: cli.build_parser().parse_args(["--test_path", str(tmp_path), "--synthetic", "tiny"] + list(extra))
    assert cli.apply_degrade(parse()) is None
    with pytest.raises(SystemExit, match="needs --degrade"):
        cli.apply_degrade(parse("--degrade_seed", "3"))
    with pytest.raises(SystemExit, match="preset"):
        cli.apply_degrade(parse("--degrade", "esrgan"))
    with pytest.raises(SystemExit, match="must be >= 0"):
        cli.apply_degrade(parse("--degrade", "bicubic", "--degrade_seed", "-1"))
    broken = tmp_path / "broken.json"
    broken.write_text("{\"stages\": [{\"scale\": -1}]}")
    with pytest.raises(SystemExit, match="recipe JSON"):
        cli.apply_degrade(parse("--degrade", str(broken)))
    small = tmp_path / "small.json"
    small.write_text(D.sample_recipe("bicubic", 0, resize_lq=False).to_json())
    with pytest.raises(SystemExit, match="resize_lq"):
        cli.apply_degrade(parse("--degrade", str(small)))                 # --gt_path defaults to --test_path
    a = parse("--degrade", str(small), "--input_fidelity")
    assert cli.apply_degrade(a) == {"spec": str(small), "seed": 0} and a.gt_path is None
    a = parse("--degrade", "realesrgan", "--degrade_seed", "5")
    assert cli.apply_degrade(a) == {"spec": "realesrgan", "seed": 5} and a.gt_path == str(tmp_path)
    assert cli.apply_metrics(a)["gt_path"] == str(tmp_path)
    # a refusal comes before the weights load
    a = parse("--degrade_seed", "3")
    with pytest.raises(SystemExit, match="needs --degrade"):
        cli.main(a, "cpu")
