"""GPU: device-side PSNR / SSIM (ops.image_metrics / iir_image_metrics) against the fp64 restatement of the contract and the
fp32 restatement of the kernel's own arithmetic (tests/metrics_ref.py), its determinism, and the `instantir_amd.metrics` and CLI
wiring.

Bounds (set by the contract and the rounding points, DESIGN.md section 7 "Image metrics", not by what the kernel gives):
  MSE of two 8-bit sources (uint8 or quantised) without y_channel: EQUAL to the fp64 restatement -- integer squares below 2^16,
      at most 8 per thread in fp32 (below 2^24), fp64 from there, one division.
  every other MSE and every SSIM: |kernel - fp64 restatement| <= metrics_ref.bounds(...), the worst case over the rounding of
      the pixel pipeline, the taps, 11 fmaf per axis, the cancellation in E[x^2] - mu^2 about the pivot 128, the map's products
      and division and the per-thread sums;
  and |kernel - fp32 restatement| <= 4 x 2^-24 of the figure: the restatement rounds where the kernel rounds, so what is left
      is the order of the fp64 additions -- a slip in a tap, an index or a mask shows here long before the worst-case bound.
Shapes (T = 32): one window; one tile edge crossed in x with a ragged end and two images; both axes crossed into the halo of a
second tile; a crop that is a multiple of nothing.  Every operand lies inside a larger buffer: NaN around an fp32 source, the
byte 255 around a uint8 source whose content stays below 251."""
import json
import math

import numpy as np
import pytest
import torch

import metrics_ref as R

pytestmark = pytest.mark.gpu

ULPS = 4 * 2.0 ** -24
PAD = 4096
_shape_id = lambda sc: "x".join(map(str, sc[0])) + f"-crop{sc[1]}"


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from instantir_amd import lib
    lib.load()
    return torch.device("cuda:0")


def _log(name, value):
    from conftest import record_psnr
    record_psnr("metrics." + name, value)


def _guarded(x, dev):
    """`x` on the device as a view into a larger buffer: NaN around fp32, 255 around uint8."""
    t = torch.from_numpy(x)
    if x.dtype == np.uint8:
        assert x.max() < 255
        buf = torch.full((t.numel() + 2 * PAD,), 255, dtype=torch.uint8, device=dev)
    else:
        buf = torch.full((t.numel() + 2 * PAD,), float("nan"), device=dev)
    view = buf[PAD:PAD + t.numel()].view(t.shape)
    view.copy_(t)
    return view, buf


def _pair(seed, shape, a_u8, b_u8):
    a, b = R.pair(seed, shape, a_u8, b_u8)
    return tuple(np.minimum(x, 250) if x.dtype == np.uint8 else x for x in (a, b))


_REF = {}


def _reference(si, form, y):
    """(a, b, fp64 figures, fp32-restatement figures for both / psnr only / ssim only), computed once per case."""
    key = (si, form, y)
    if key not in _REF:
        shape, c = R.GPU_SHAPES[si]
        a_u8, b_u8, q = R.SOURCE_FORMS[form]
        a, b = _pair(11 + si, shape, a_u8, b_u8)
        _REF[key] = (a, b, R.evaluate(a, b, c, y, q), {w: R.evaluate32(a, b, c, y, q, what=w) for w in (("psnr", "ssim"), ("psnr",), ("ssim",))})
    return _REF[key]


# ---- the kernel against the restatements ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("y", [False, True], ids=["rgb", "y"])
@pytest.mark.parametrize("form", sorted(R.SOURCE_FORMS))
@pytest.mark.parametrize("si", range(len(R.GPU_SHAPES)), ids=[_shape_id(s) for s in R.GPU_SHAPES])
def test_figures_match_both_restatements(dev, si, form, y):
    from instantir_amd import ops
    shape, c = R.GPU_SHAPES[si]
    if y and shape[1] != 3:
        with pytest.raises(ValueError, match="y_channel"):
            ops.image_metrics(torch.zeros(shape, device=dev), torch.zeros(shape, device=dev), y_channel=True)
        return
    a_u8, b_u8, q = R.SOURCE_FORMS[form]
    a, b, want, want32 = _reference(si, form, y)
    (ta, bufa), (tb, bufb) = _guarded(a, dev), _guarded(b, dev)
    b_mse, b_ssim = R.bounds(a_u8 or q[0], b_u8 or q[1], y)
    exact = (a_u8 or q[0]) and (b_u8 or q[1]) and not y
    worst = [0.0, 0.0]
    for what in (("psnr", "ssim"), ("psnr",), ("ssim",)):
        got = ops.image_metrics(ta, tb, crop_border=c, y_channel=y, quantize=q, what=what)
        torch.cuda.synchronize()
        assert got.dtype == torch.float64 and got.shape == (shape[0], 2) and got.device == ta.device
        got = got.cpu().numpy()
        ref32 = want32[what]
        if "psnr" in what:
            err = np.abs(got[:, 0] - want[:, 0]).max()
            print(f"mse {_shape_id(R.GPU_SHAPES[si])} {form} y={int(y)} {'+'.join(what)} max_abs_err {err:.3e} bound {b_mse:.3e} "
                  f"vs fp32 restatement {np.abs(got[:, 0] - ref32[:, 0]).max():.3e}")
            worst[0] = max(worst[0], err / b_mse)
            if exact:
                assert np.array_equal(got[:, 0], want[:, 0]), (got[:, 0], want[:, 0])
            assert err <= b_mse, (what, err, b_mse)
            assert (np.abs(got[:, 0] - ref32[:, 0]) <= ULPS * np.abs(ref32[:, 0])).all(), (what, got[:, 0], ref32[:, 0])
        else:
            assert np.isnan(got[:, 0]).all()
        if "ssim" in what:
            err = np.abs(got[:, 1] - want[:, 1]).max()
            print(f"ssim {_shape_id(R.GPU_SHAPES[si])} {form} y={int(y)} {'+'.join(what)} max_abs_err {err:.3e} bound {b_ssim:.3e} "
                  f"vs fp32 restatement {np.abs(got[:, 1] - ref32[:, 1]).max():.3e}")
            worst[1] = max(worst[1], err / b_ssim)
            assert err <= b_ssim, (what, err, b_ssim)
            assert (np.abs(got[:, 1] - ref32[:, 1]) <= ULPS * np.abs(ref32[:, 1])).all(), (what, got[:, 1], ref32[:, 1])
            assert (np.abs(want[:, 1]) > 0.05).all()                     # pictures, not noise: a figure the ulp test can hold on to
        else:
            assert np.isnan(got[:, 1]).all()
    tag = f"{_shape_id(R.GPU_SHAPES[si])}_{form}_{'y' if y else 'rgb'}"
    print(f"ratio {tag} mse_err_over_bound {worst[0]:.3e} ssim_err_over_bound {worst[1]:.3e}")
    _log(tag + ".mse_err_over_bound_1e-6", 1e6 * worst[0])
    _log(tag + ".ssim_err_over_bound_1e-6", 1e6 * worst[1])
    for buf, t in ((bufa, ta), (bufb, tb)):                              # the guard bands are as they were
        edge = torch.cat([buf[:PAD], buf[PAD + t.numel():]])
        assert (edge == 255).all() if buf.dtype == torch.uint8 else torch.isnan(edge).all()


def test_identical_images_and_a_constant_offset(dev):
    from instantir_amd import metrics as M, ops
    a, _ = R.pair(3, (2, 3, 40, 50), True, True)
    ta = torch.from_numpy(a).to(dev)
    got = ops.image_metrics(ta, ta.clone()).cpu().numpy()
    assert np.array_equal(got[:, 0], [0.0, 0.0]) and np.abs(got[:, 1] - 1.0).max() <= 4 * 2.0 ** -24
    assert M.psnr(a, a, device=dev) == [math.inf, math.inf]
    base = np.minimum(a, 200)
    for d in (1, 7, 50):
        assert np.abs(np.array(M.psnr(base, base + np.uint8(d), device=dev)) - 20 * math.log10(255 / d)).max() < 1e-12
    ab, ba = ops.image_metrics(ta, torch.from_numpy(base).to(dev)), ops.image_metrics(torch.from_numpy(base).to(dev), ta)
    assert torch.equal(ab[:, 0], ba[:, 0]) and (ab[:, 1] - ba[:, 1]).abs().max().item() <= 4 * 2.0 ** -24


def test_workspace_argument(dev):
    from instantir_amd import ops
    a, b = (torch.from_numpy(x).to(dev) for x in R.pair(5, (1, 3, 43, 44), True, True))
    want = ops.image_metrics(a, b)
    ws = torch.full((2 * 3 * 4 + 8,), float("nan"), dtype=torch.float64, device=dev)
    assert torch.equal(ops.image_metrics(a, b, ws=ws[:24]), want) and torch.isnan(ws[24:]).all()
    with pytest.raises(ValueError, match="ws needs 192"):
        ops.image_metrics(a, b, ws=ws[:23])
    with pytest.raises(ValueError, match="ws needs"):
        ops.image_metrics(a, b, ws=torch.zeros(64, dtype=torch.float64))


# ---- determinism -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 3, 11, 11), (2, 3, 75, 70), (1, 3, 512, 384)], ids=lambda s: "x".join(map(str, s)))
def test_repeat_and_busy_neighbour_give_the_same_bits(dev, shape):
    from instantir_amd import ops
    a, b = R.pair(9, shape, False, True)
    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    keep = ta.clone()
    runs = lambda: [ops.image_metrics(ta, tb, y_channel=y, what=w) for y in (False, True) for w in (("psnr", "ssim"), ("psnr",))]
    first, again = runs(), runs()
    torch.cuda.synchronize()
    same = lambda p, q: all(torch.equal(x.view(torch.int64), z.view(torch.int64)) for x, z in zip(p, q))
    assert same(first, again), "two runs differ"
    assert torch.equal(ta, keep), "a source was modified"
    side = torch.cuda.Stream()
    m = torch.randn(2048, 2048, device=dev, dtype=torch.half)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(24):
            m = (m @ m).clamp_(-1, 1)
    busy = runs()
    torch.cuda.synchronize()
    assert same(first, busy), "a run beside a busy stream differs"


# ---- the module ------------------------------------------------------------------------------------------------------------------
def test_evaluate_gives_the_same_floats_for_every_form_of_one_pair(dev):
    from PIL import Image
    from instantir_amd import metrics as M, ops
    a, b = R.pair(21, (2, 3, 40, 52), True, True)
    raw = ops.image_metrics(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), crop_border=2).cpu().tolist()
    want = M.evaluate(a, b, crop_border=2, device=dev)
    assert want["psnr"] == [M.psnr_from_mse(r[0]) for r in raw] and want["ssim"] == [r[1] for r in raw]
    assert set(want) == {"psnr", "ssim", "psnr_mean", "ssim_mean"} and all(isinstance(v, float) for v in want["psnr"] + want["ssim"])
    assert want["psnr_mean"] == sum(want["psnr"]) / 2 and want["ssim_mean"] == sum(want["ssim"]) / 2
    pil = lambda x: [Image.fromarray(i) for i in x]
    as_f = lambda x: (torch.from_numpy(x).permute(0, 3, 1, 2).float() / 255)
    forms = [(pil(a), pil(b)), (torch.from_numpy(a), pil(b)), (a, torch.from_numpy(b).to(dev))]
    for fa, fb in forms:
        assert M.evaluate(fa, fb, crop_border=2, device=dev) == want
    # [0, 1] forms of the same 8-bit images: the same figures once they are quantised, as the saved file would be
    for fa, fb in ((as_f(a), b), (as_f(a).to(dev), as_f(b)), (as_f(a).permute(0, 2, 3, 1).numpy(), pil(b))):
        assert M.evaluate(fa, fb, crop_border=2, quantize=True, device=dev) == want
    one = M.evaluate(pil(a)[1], b[1], crop_border=2, device=dev)
    assert one["psnr"] == want["psnr"][1:] and one["ssim"] == want["ssim"][1:]
    assert M.psnr(pil(a)[1], b[1], crop_border=2, device=dev) == want["psnr"][1]
    assert M.ssim(a, b, crop_border=2, device=dev) == want["ssim"]
    y = M.evaluate(a, b, y_channel=True, metrics="ssim", device=dev)
    assert set(y) == {"ssim", "ssim_mean"} and y["ssim"] != want["ssim"]
    grey = M.evaluate(a[0, :, :, 0], b[0, :, :, 0], device=dev)
    assert grey["psnr"] == [M.psnr_from_mse(R.evaluate(a[:1, :, :, :1], b[:1, :, :, :1])[0, 0])]


def test_input_fidelity_is_a_resample_followed_by_the_metrics(dev):
    from PIL import Image
    from instantir_amd import metrics as M, ops
    restored, _ = R.pair(31, (1, 3, 96, 80), True, True)
    lq_same, _ = R.pair(32, (1, 3, 96, 80), True, True)
    lq_small, _ = R.pair(33, (1, 3, 40, 36), True, True)
    up = lambda x: torch.from_numpy(x).to(dev)

    def figures(t):
        rows = t.cpu().tolist()
        return {"psnr": [M.psnr_from_mse(r[0]) for r in rows], "ssim": [r[1] for r in rows]}

    same = M.input_fidelity(Image.fromarray(restored[0]), Image.fromarray(lq_same[0]), device=dev)
    want = figures(ops.image_metrics(ops.resample(up(restored), (96, 80), "bicubic", quantize=True, scale=1 / 255.0), up(lq_same), quantize=(True, False)))
    assert {k: same[k] for k in want} == want == figures(ops.image_metrics(up(restored), up(lq_same)))
    for flt in ("bicubic", "lanczos"):
        got = M.input_fidelity(restored, lq_small, filter=flt, device=dev)
        small = ops.resample(up(restored), (40, 36), flt, quantize=True, scale=1 / 255.0)
        want = figures(ops.image_metrics(small, up(lq_small), quantize=(True, False)))
        assert {k: got[k] for k in want} == want and got["psnr_mean"] == want["psnr"][0]
        q = ops.resample(up(restored), (40, 36), flt, quantize=True)
        assert want == figures(ops.image_metrics(q.permute(0, 2, 3, 1).to(torch.uint8).contiguous(), up(lq_small)))     # the 8-bit image itself
    # a float restoration: float mode, clamped to [0, 1], nothing rounded
    rf = torch.from_numpy(restored).permute(0, 3, 1, 2).float().div(255).contiguous()
    got = M.input_fidelity(rf, lq_small, metrics="psnr", crop_border=1, device=dev)
    want = ops.image_metrics(ops.resample(rf.to(dev), (40, 36), "bicubic", clamp=(0.0, 1.0)), up(lq_small), crop_border=1, what="psnr")
    assert got == {"psnr": [M.psnr_from_mse(want[0, 0].item())], "psnr_mean": M.psnr_from_mse(want[0, 0].item())}


# ---- the CLI ---------------------------------------------------------------------------------------------------------------------
def test_cli_metrics_json_equals_the_python_api_on_the_saved_files(tmp_path, dev):
    from PIL import Image
    import instantir_amd.infer as cli
    from instantir_amd import metrics as M
    src, gt, plain, scored = tmp_path / "in", tmp_path / "gt", tmp_path / "plain", tmp_path / "scored"
    src.mkdir(); gt.mkdir()
    rng = np.random.default_rng(0)
    for i, n in enumerate(("a.png", "b.png")):
        Image.fromarray(rng.integers(0, 255, (96, 96, 3), dtype=np.uint8)).save(src / n)
        Image.fromarray(R.as_u8(R.picture(40 + i, 1, 3, 128, 128))[0]).save(gt / n)
    common = ["--test_path", str(src), "--synthetic", "tiny", "--num_inference_steps", "2", "--width", "128", "--height", "128",
              "--batch_size", "2", "--cfg", "5.0"]
    flags = ["--gt_path", str(gt), "--input_fidelity", "--metrics_crop", "3", "--metrics_y"]
    orig = cli.resize_img
    cli.resize_img = lambda im, **kw: orig(im, max_side=128, min_side=128, **kw)      # keep the tiny nets tiny
    try:
        torch.manual_seed(123)          # the VAE posterior sample draws from the global RNG
        cli.main(cli.build_parser().parse_args(common + ["--out_path", str(plain)]), dev)
        torch.manual_seed(123)
        cli.main(cli.build_parser().parse_args(common + ["--out_path", str(scored)] + flags), dev)
    finally:
        cli.resize_img = orig
    assert sorted(p.name for p in plain.iterdir()) == ["a.png", "b.png"]                 # without the flags: no report
    assert sorted(p.name for p in scored.iterdir()) == ["a.png", "b.png", "metrics.json"]
    for n in ("a.png", "b.png"):
        assert (plain / n).read_bytes() == (scored / n).read_bytes(), n
    rep = json.load(open(scored / "metrics.json"))
    assert rep["settings"] == {"gt_path": str(gt), "input_fidelity": True, "metrics": ["psnr", "ssim"], "y_channel": True, "crop_border": 3}
    for n in ("a.png", "b.png"):
        saved = Image.open(scored / n).convert("RGB")
        want = M.evaluate(saved, Image.open(gt / n).convert("RGB"), crop_border=3, y_channel=True, device=dev)
        fid = M.input_fidelity(saved, Image.open(src / n).convert("RGB"), crop_border=3, y_channel=True, device=dev)
        assert rep["files"][n] == {"psnr": want["psnr"][0], "ssim": want["ssim"][0], "input_psnr": fid["psnr"][0], "input_ssim": fid["ssim"][0]}
    assert rep["mean"]["psnr"] == (rep["files"]["a.png"]["psnr"] + rep["files"]["b.png"]["psnr"]) / 2
    assert set(rep["mean"]) == {"psnr", "ssim", "input_psnr", "input_ssim"}
