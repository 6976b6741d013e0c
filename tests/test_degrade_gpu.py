"""GPU: the three degradation launches (`ops.filter2d`, `ops.add_gaussian_noise`, `ops.jpeg_roundtrip`) element-wise against
the fp64 restatements of tests/degrade_ref.py inside the derived bounds, NaN guard bands around every operand, two launches
bit-equal; `degrade()` stage by stage; and `infer --degrade`."""
import json

import numpy as np
import pytest
import torch

import degrade_ref as R
from loop_ref import dev  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

GUARD = 4099                       # fp32 elements of NaN on either side of every operand (odd: the planes start 4-byte aligned only)


def _embedded(a, dev, fill=None):
    """numpy fp32 array -> a contiguous device tensor of its shape in the middle of a NaN-filled allocation: (view, buffer)"""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    buf = torch.full((t.numel() + 2 * GUARD,), float("nan"), dtype=torch.float32, device=dev)
    view = buf[GUARD:GUARD + t.numel()].view(t.shape)
    view.copy_(t if fill is None else torch.full_like(t, fill))
    return view, buf


def _guards_intact(*bufs):
    return all(bool(torch.isnan(b[:GUARD]).all() and torch.isnan(b[-GUARD:]).all()) for b in bufs)


def _twice(dev, launch, x, *operands):
    """launch(x_d, *operand_d, out_d) twice on guarded operands: the inputs keep their bits, the guards stay NaN, the two
    outputs are bit-equal -> the output as fp32 numpy"""
    outs = []
    for _ in range(2):
        x_d, bx = _embedded(x, dev)
        ops_d = [_embedded(o, dev) for o in operands]
        out_d, bo = _embedded(x, dev, fill=7.0)
        launch(x_d, *[o[0] for o in ops_d], out_d)
        torch.cuda.synchronize()
        assert _guards_intact(bx, bo, *[o[1] for o in ops_d])
        assert np.array_equal(x_d.cpu().numpy(), x)
        outs.append(out_d.cpu().numpy())
    assert outs[0].tobytes() == outs[1].tobytes()
    return outs[0]


# ---- filter2d ---------------------------------------------------------------------------------------------------------------
def _kernels(n, k, seed):
    """n asymmetric k x k kernels with a few negative taps, sum 1: a transposed or flipped tap index moves the result"""
    g = np.random.default_rng(seed)
    t = g.random((n, k, k)) ** 3 - 0.05
    t[:, 0, -1] += 0.5                                  # no symmetry of any kind
    return (t / t.sum(axis=(1, 2), keepdims=True)).astype(np.float32)


def _check_filter(dev, x, taps):
    from instantir_amd import ops
    got = _twice(dev, lambda x_d, t_d, o_d: ops.filter2d(x_d, t_d, out=o_d), x, taps)
    want, like = R.filter2d64(x, taps), R.filter2d32(x, taps)
    err, tol = np.abs(got - want), R.filter2d_bound(x, taps)
    d32, tol32 = np.abs(got - like), R.filter2d_bound32(x, taps)
    print(f"filter2d {x.shape} k {taps.shape[-1]}: largest |error| / bound {(err / tol).max():.3f} (bound {tol.max():.3e}); against the fp32 "
          f"restatement {int((got != like).sum())} of {got.size} differ, largest / allowed {(d32 / tol32).max():.3f}")
    assert np.isfinite(got).all() and (err <= tol).all() and (d32 <= tol32).all()
    return got


def test_filter2d_smallest_image_per_image_kernels(dev):
    """(2, 3, 11, 13) with k = 21: the reflection reaches almost across the image; each image has a kernel of its own"""
    x = np.random.default_rng(1).random((2, 3, 11, 13), dtype=np.float32)
    taps = _kernels(2, 21, 2)
    got = _check_filter(dev, x, taps)
    swapped = R.filter2d64(x, taps[::-1])
    assert (np.abs(got - swapped) > 100 * R.filter2d_bound(x, taps)).any()      # the other image's kernel gives something else


def test_filter2d_ragged_tiles_and_zero_padded_kernel(dev):
    """(1, 3, 37, 67): tile edges crossed raggedly on both axes; k = 7 and the same kernel zero-padded to 21 agree"""
    x = np.random.default_rng(3).random((1, 3, 37, 67), dtype=np.float32)
    taps = _kernels(1, 7, 4)
    padded = np.pad(taps, ((0, 0), (7, 7), (7, 7)))
    a, b = _check_filter(dev, x, taps), _check_filter(dev, x, padded)
    assert (np.abs(a - b) <= R.filter2d_bound(x, taps) + R.filter2d_bound(x, padded)).all()
    transposed = R.filter2d64(x, taps.transpose(0, 2, 1))
    assert (np.abs(a - transposed) > 100 * R.filter2d_bound(x, taps)).any()


def test_filter2d_identity_keeps_the_bits(dev):
    x = np.random.default_rng(5).random((1, 1, 32, 32), dtype=np.float32)
    got = _check_filter(dev, x, np.ones((1, 1, 1), np.float32))
    assert got.tobytes() == x.tobytes()


# ---- noise ------------------------------------------------------------------------------------------------------------------
NOISE_SHAPE = (2, 3, 19, 23)


def _noise(dev, x, sigma, seed, stream=0, gray=False):
    from instantir_amd import ops
    return _twice(dev, lambda x_d, o_d: ops.add_gaussian_noise(x_d, sigma, seed, stream=stream, gray=gray, out=o_d), x)


def test_noise_z_stays_inside_the_ulp_budget(dev):
    """The kernel's z itself: with x = 0 and sigma / 255 = 1 / 8 the launch returns z / 8 exactly wherever z > 0.  Its relative
    distance from the fp64 restatement, in units of 2^-23, is printed; R.NOISE_Z_ULPS = 3.3 is twice the largest figure measured
    on an MI355X over these samples, 1.611 (DESIGN.md section 7 "Synthetic degradation"; no per-function ulp table of the device
    math library is at hand)."""
    shape = (1, 3, 128, 171)
    got = _noise(dev, np.zeros(shape, np.float32), 31.875, seed=11)
    z = R.normal64(shape, 11)
    pos = z > 1e-3
    assert (got[~(z > 0)] == 0).all() and (got[pos] > 0).all()
    rel = np.abs(got[pos].astype(np.float64) * 8.0 - z[pos]) / z[pos] / 2.0 ** -23
    print(f"noise: z over {int(pos.sum())} samples: largest relative error {rel.max():.3f} ulp, budget {R.NOISE_Z_ULPS}")
    assert rel.max() <= R.NOISE_Z_ULPS


@pytest.mark.parametrize("gray", [False, True])
@pytest.mark.parametrize("sigma", [25.0, (0.0, 50.0)])
def test_noise_matches_fp64(dev, sigma, gray):
    x = np.random.default_rng(7).random(NOISE_SHAPE, dtype=np.float32)
    x[0, 0, 0, :4] = (-0.25, 0.0, 1.0, 1.5)                                  # values the clamp has to catch
    x[1, 2, -1, :4] = (-0.25, 0.0, 1.0, 1.5)
    sig = np.broadcast_to(np.asarray(sigma, np.float32), (2,))
    got = _noise(dev, x, sigma, seed=(7 << 32) | 5, stream=3, gray=gray)
    want, raw = R.noise64(x, sig, (7 << 32) | 5, 3, gray)
    tol = np.broadcast_to(R.noise_bound(x, sig, R.NOISE_Z_ULPS), x.shape)
    near = (np.abs(raw) <= tol) | (np.abs(raw - 1.0) <= tol)                # compared after clamping only: the same comparison
    err = np.abs(got - want)
    print(f"noise sigma {sigma} gray {gray}: largest |error| / bound {(err[tol > 0] / tol[tol > 0]).max():.3f}, {int(near.sum())} element(s) at a clamp")
    assert (err <= tol).all() and got.min() >= 0.0 and got.max() <= 1.0
    for n in range(2):
        if sig[n] == 0:
            assert got[n].tobytes() == np.clip(x[n], 0, 1).tobytes()


def test_noise_streams_and_seeds_differ(dev):
    x = np.full(NOISE_SHAPE, 0.5, np.float32)
    a, b, c = _noise(dev, x, 25.0, 3, stream=0), _noise(dev, x, 25.0, 3, stream=1), _noise(dev, x, 25.0, 4, stream=0)
    assert (a != b).all() and (a != c).all()
    g = _noise(dev, x, 25.0, 3, gray=True)
    assert np.array_equal(g[:, 0], g[:, 1]) and np.array_equal(g[:, 0], g[:, 2]) and np.array_equal(g[:, 0], a[:, 0])
    from instantir_amd import ops
    t = torch.from_numpy(x).to(dev)
    assert ops.add_gaussian_noise(t, 25.0, 3, out=t) is t and np.array_equal(t.cpu().numpy(), a)         # in place


# ---- JPEG -------------------------------------------------------------------------------------------------------------------
def _jpeg(dev, x, quality):
    from instantir_amd import ops
    return _twice(dev, lambda x_d, o_d: ops.jpeg_roundtrip(x_d, quality, out=o_d), x)


@pytest.mark.parametrize("quality", [(30.0, 95.0), (49.5, 50.0)])
def test_jpeg_exact_inputs_every_element(dev, quality):
    """Inputs built in the transform domain, every coefficient at least 0.15 of a step from a rounding tie: no exclusions."""
    x = R.exact_jpeg_input((2, 3, 32, 48), quality, seed=5)
    res = R.jpeg64(x, quality)
    assert res["tie_y"].min() > 0.1 and res["tie_c"].min() > 0.1
    got = _jpeg(dev, x, list(quality))
    ratio = np.abs(got - res["out"]) / res["err"]
    print(f"jpeg exact q {quality}: largest |error| / bound {ratio.max():.3f} (largest bound {res['err'].max():.3e})")
    assert (ratio <= 1.0).all()
    assert got.tobytes() != x.tobytes() and np.abs(got - x).max() < 0.2
    from instantir_amd import ops
    t = torch.from_numpy(x).to(dev)
    assert ops.jpeg_roundtrip(t, list(quality), out=t) is t and t.cpu().numpy().tobytes() == got.tobytes()      # in place


# seeds for which the fp64 restatement alone leaves at most 10 % of an image's blocks near a tie at every quality below; shares
# left out at q = 30, 50, 75, 95 (the worse image of a batch): (1,3,16,16) seed 1: 0, 0, 0, 0; (1,3,17,33) seed 3: 0, 0, 0, 0;
# (2,3,40,56) seed 4: 0.021, 0, 0, 0.083
NATURAL = [((1, 3, 16, 16), 1), ((1, 3, 17, 33), 3), ((2, 3, 40, 56), 4)]


@pytest.mark.parametrize("q", [30.0, 50.0, 75.0, 95.0])
@pytest.mark.parametrize("shape,seed", NATURAL)
def test_jpeg_natural_inputs(dev, shape, seed, q):
    """Seeded smooth-plus-noise 8-bit images: one MCU; one pixel past an MCU on both axes (edge replication); a batch.  A block
    with a coefficient within tau of a tie in the fp64 restatement is left out (a chroma block with its MCU); at most 10 % may
    be; everything else is compared element-wise."""
    x = R.smooth_noise_image(shape, seed).astype(np.float32) / np.float32(255.0)
    res = R.jpeg64(x, [q] * shape[0])
    keep, share = R.jpeg_keep_mask(res, *shape[2:])
    assert share.max() <= 0.10, share
    got = _jpeg(dev, x, q)
    ratio = np.abs(got - res["out"]) / res["err"]
    kept = np.broadcast_to(keep[:, None], got.shape)
    print(f"jpeg natural {shape} q {q}: left out {share.max():.3f}; largest |error| / bound kept {ratio[kept].max():.3f}, overall {ratio.max():.3f}")
    assert (ratio[kept] <= 1.0).all()


# ---- degrade() ----------------------------------------------------------------------------------------------------------------
def _two_stage(seed_shift=0.0):
    from instantir_amd import degrade as D
    return D.Recipe([D.Stage(blur=D.gaussian_kernel(9, 1.4, 0.8, 0.5), scale=0.75, resize_filter="bilinear", noise_sigma=12.0 + seed_shift,
                             gray_noise=False, jpeg_quality=60.0 + seed_shift),
                     D.Stage(blur=D.plateau_kernel(7, 1.1, 1.5), scale=0.3, resize_filter="bicubic", noise_sigma=6.0, gray_noise=True,
                             jpeg_quality=80.0)],
                    final_sinc=D.sinc_kernel(7, 2.0), jpeg_before_final_resize=False, sf=4, resize_lq=True, final_filter="bilinear")


def test_degrade_stage_by_stage(dev):
    """Each stage's device output against the fp64 restatement applied to the device's own input of that stage, with per-image
    recipes (kernels, sigmas and qualities differ between the two images)."""
    import dataclasses
    from instantir_amd import degrade as D
    clean = R.smooth_noise_image((2, 3, 64, 96), 9)
    recipes = [_two_stage(), _two_stage(5.0)]
    lq, trace = D.degrade(clean.transpose(0, 2, 3, 1), recipes, seed=21, device=dev, return_stages=True)
    labels = [l for l, _ in trace]
    assert labels == ["stage0.blur", "stage0.resize", "stage0.noise", "stage0.jpeg", "stage1.blur", "stage1.resize", "stage1.noise",
                      "final.resize", "final.sinc", "stage1.jpeg", "out"]
    assert tuple(lq.shape) == (2, 3, 64, 96) and lq.dtype == torch.float32 and 0.0 <= float(lq.min()) and float(lq.max()) <= 1.0
    assert tuple(dict(trace)["stage0.resize"].shape[-2:]) == (48, 72) and tuple(dict(trace)["final.sinc"].shape[-2:]) == (16, 24)
    prev = (torch.from_numpy(clean).to(dev).float() / 255.0).cpu().numpy()
    for label, t in trace:
        got = t.cpu().numpy()
        stage, part = label.split(".") if "." in label else (None, label)
        i = int(stage[5:]) if stage and stage.startswith("stage") else None
        if part == "blur" or part == "sinc":
            ks = [(r.stages[i].blur if part == "blur" else r.final_sinc) for r in recipes]
            taps = np.stack([D.pad_kernel(k, max(k.shape[0] for k in ks)) for k in ks]).astype(np.float32)
            assert (np.abs(got - R.filter2d64(prev, taps)) <= R.filter2d_bound(prev, taps)).all(), label
        elif part == "noise":
            sig = np.array([r.stages[i].noise_sigma for r in recipes], np.float32)
            want, _ = R.noise64(prev, sig, 21, i, recipes[0].stages[i].gray_noise)
            assert (np.abs(got - want) <= R.noise_bound(prev, sig, R.NOISE_Z_ULPS)).all(), label
        elif part == "jpeg":
            res = R.jpeg64(prev, np.array([r.stages[i].jpeg_quality for r in recipes], np.float32))
            keep, share = R.jpeg_keep_mask(res, *got.shape[-2:])
            kept = np.broadcast_to(keep[:, None], got.shape)
            assert share.max() <= 0.25 and (np.abs(got - res["out"])[kept] <= res["err"][kept]).all(), (label, share)
        else:
            assert got.shape[:2] == prev.shape[:2] and np.isfinite(got).all(), label            # resampling has its own tests
        prev = got
    again = D.degrade(clean.transpose(0, 2, 3, 1), recipes, seed=21, device=dev)
    other = D.degrade(clean.transpose(0, 2, 3, 1), recipes, seed=22, device=dev)
    assert torch.equal(again, lq) and not torch.equal(other, lq)
    small = D.degrade(clean.transpose(0, 2, 3, 1), [dataclasses.replace(r, resize_lq=False) for r in recipes], seed=21, device=dev)
    assert tuple(small.shape) == (2, 3, 16, 24)
    with pytest.raises(ValueError, match="share"):
        D.degrade(clean.transpose(0, 2, 3, 1), [recipes[0], dataclasses.replace(recipes[1], sf=2)], device=dev)


# ---- the CLI ----------------------------------------------------------------------------------------------------------------
def test_cli_degrade_bicubic(tmp_path, dev):
    from PIL import Image
    import instantir_amd.infer as cli
    from instantir_amd import degrade as D, metrics as M
    src, out, lq_only, again = tmp_path / "clean", tmp_path / "out", tmp_path / "lq_only", tmp_path / "again"
    src.mkdir(); lq_only.mkdir()
    clean = R.smooth_noise_image((2, 3, 128, 128), 12)
    for i, n in enumerate(("a.png", "b.png")):
        Image.fromarray(clean[i].transpose(1, 2, 0)).save(src / n)
    common = ["--synthetic", "tiny", "--num_inference_steps", "2", "--batch_size", "2", "--cfg", "5.0"]
    orig = cli.resize_img
    cli.resize_img = lambda im, **kw: orig(im, max_side=128, min_side=128, **kw)      # keep the tiny nets tiny
    try:
        torch.manual_seed(123)          # the VAE posterior sample draws from the global RNG
        cli.main(cli.build_parser().parse_args(common + ["--test_path", str(src), "--out_path", str(out), "--degrade", "bicubic",
                                                         "--degrade_seed", "7"]), dev)
        for n in ("a.png", "b.png"):
            (lq_only / n).write_bytes((out / "lq" / n).read_bytes())
        torch.manual_seed(123)
        cli.main(cli.build_parser().parse_args(common + ["--test_path", str(lq_only), "--out_path", str(again), "--gt_path", str(src)]), dev)
    finally:
        cli.resize_img = orig
    assert sorted(p.name for p in out.iterdir()) == ["a.png", "b.png", "lq", "metrics.json"]
    assert sorted(p.name for p in (out / "lq").iterdir()) == ["a.json", "a.png", "b.json", "b.png"]
    for i, n in enumerate(("a.png", "b.png")):
        recipe = D.Recipe.from_json((out / "lq" / (n[:-4] + ".json")).read_text())
        assert recipe == D.sample_recipe("bicubic", 7, n)
        want = D.quantize_u8(D.degrade([Image.open(src / n).convert("RGB")], recipe, seed=D.noise_seed(7, n), device=dev))[0]
        assert np.array_equal(np.asarray(Image.open(out / "lq" / n).convert("RGB")), want), n
        assert (out / n).read_bytes() == (again / n).read_bytes(), n
    rep, rep2 = json.load(open(out / "metrics.json")), json.load(open(again / "metrics.json"))
    assert rep["settings"]["gt_path"] == str(src) and rep["files"] == rep2["files"] and rep["mean"] == rep2["mean"]
    for n in ("a.png", "b.png"):
        want = M.evaluate(Image.open(out / n).convert("RGB"), Image.open(src / n).convert("RGB"), device=dev)
        assert rep["files"][n] == {"psnr": want["psnr"][0], "ssim": want["ssim"][0]}
