"""GPU: the DISTS kernels (ops.dists_l2pool / dists_stats / dists_image_stats), the whole network (instantir_amd.dists.DISTS) and
the CLI wiring against the fp64 restatement of the contract (tests/dists_ref.py).

Bounds (from the contract and the rounding points, DESIGN.md section 7 "DISTS", not from what the kernels give; the derivations
stand in dists_ref.py):
  l2pool: on the same 16-bit pre-activations, |out - exact| <= 1.001 (5.5 u + ROUNDING[dt]) exact + TINY[dt], u = 2^-24: eight
          fp32 additions of non-negative exact terms and the + 1e-12 (9 u on the sum), halved by the square root, which rounds
          once, then one rounding of the 16-bit type (absolute below its smallest normal number).
  stats:  each of the five sums within 1.001 (n - 1) 2^-53 sum |terms| of the long-double sum of the same values: every product
          is exact in fp64, so this is the summation's error alone, and it leaves no room for an fp32 partial.
  net:    per dtype and stage, both terms within 3 x e_model; e_model = the largest |restatement(storage = dtype) -
          restatement(fp64)| over the three cases, the stage's two terms and both conv accumulation types of the restatement
          (fp32 and fp64), measured on the CPU here (the factor 3: a third summation order inside the MFMA tiles).  Stage 0
          never sees a 16-bit type: 1e-12.
Every figure is printed before its assertion (run with -s to keep them; profiles/dists_test_figures.log is such a run).
Every operand lies inside a larger buffer filled with NaN."""
import json

import numpy as np
import pytest
import torch

import dists_ref as R

pytestmark = pytest.mark.gpu

PAD = 4096
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}
SIZES = [(5, 7), (16, 16), (37, 53), (1, 1)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from instantir_amd import lib
    lib.load()
    return torch.device("cuda:0")


def _log(line):
    print(line)


def _guarded(t, dev, fill=float("nan")):
    """`t` on the device as a view into a larger buffer of `fill`; (view, buffer)."""
    buf = torch.full((t.numel() + 2 * PAD,), fill, dtype=t.dtype, device=dev)
    view = buf[PAD:PAD + t.numel()].view(t.shape)
    view.copy_(t)
    return view, buf


def _bands_intact(buf, n):
    """The guard bands of a `_guarded` NaN buffer around n elements are still NaN."""
    return bool(torch.isnan(buf[:PAD]).all()) and bool(torch.isnan(buf[PAD + n:]).all())


def _bits(t):
    return t.contiguous().view(torch.int16)


def _nchw(x):
    """(images, H, W, C) 16-bit pre-activations -> the fp64 (images, C, H, W) feature after the ReLU."""
    return x.double().clamp_min(0.0).permute(0, 3, 1, 2)


# ---- l2pool ---------------------------------------------------------------------------------------------------------------------
def _pool_inputs(C, H, W, dt):
    """Gaussian pre-activations (about half negative) of two images as (2, H, W, C) in `dt`; the whole 3x3 window of output pixel
    (1, 1) of image 0 non-positive (a 1 x 1 image: all of image 1), and a large value in the last row and column."""
    g = torch.Generator().manual_seed(C * 1000 + H * 10 + W)
    x = torch.randn(2, H, W, C, generator=g).to(dt)
    if min(H, W) >= 4:
        x[0, 1:4, 1:4] = -x[0, 1:4, 1:4].abs()
    else:
        x[1] = -x[1].abs()
    x[0, H - 1, W - 1, 0] = 3.0
    return x


def _run_pool(x, H, W, dev, extra=8):
    """-> the (rows, C) output, taken as the first C columns of a matrix `extra` columns wider whose other columns hold 7."""
    from instantir_amd import ops
    C = x.shape[-1]
    xv, xbuf = _guarded(x.reshape(-1, C), dev)
    rows = 2 * ((H + 1) // 2) * ((W + 1) // 2)
    wide, obuf = _guarded(torch.full((rows, C + extra), 7.0, dtype=x.dtype), dev)
    wide[:, :C] = float("nan")
    out = ops.dists_l2pool(xv, 2, H, W, out=wide[:, :C])
    torch.cuda.synchronize()
    assert out.data_ptr() == wide.data_ptr()
    assert torch.equal(_bits(xv.cpu()), _bits(x.reshape(-1, C))) and _bands_intact(xbuf, x.numel())          # the input is unchanged
    assert _bands_intact(obuf, wide.numel()) and bool((wide[:, C:] == 7.0).all())                            # columns past C keep their bits
    return wide[:, :C].cpu()


@pytest.mark.parametrize("name", sorted(DTYPES))
@pytest.mark.parametrize("C", [64, 128, 256, 512])
def test_l2pool_against_fp64(dev, C, name):
    dt = DTYPES[name]
    floor = torch.tensor(1e-12, dtype=torch.float32).sqrt().to(dt)                   # the 16-bit rounding of 1e-6
    for H, W in SIZES:
        x = _pool_inputs(C, H, W, dt)
        exact = R.l2pool(_nchw(x)).permute(0, 2, 3, 1).reshape(-1, C)
        got = _run_pool(x, H, W, dev)
        assert bool(torch.isfinite(got).all())
        err, bound = (got.double() - exact).abs(), R.l2pool_bound(exact, dt)
        _log(f"l2pool {name} C={C} {H}x{W}: max err / bound {float((err / bound).max()):.4f}; out in [{float(got.min()):.3e}, {float(got.max()):.3e}]")
        assert bool((err <= bound).all())
        oh, ow = (H + 1) // 2, (W + 1) // 2
        planted = got.view(2, oh, ow, C)[0, 1, 1] if min(H, W) >= 4 else got.view(2, oh, ow, C)[1, 0, 0]
        assert torch.equal(_bits(planted), _bits(floor.expand(C)))                   # sqrt(0 + 1e-12)
        assert float(got.view(2, oh, ow, C)[0, oh - 1, ow - 1, 0]) > 0.5             # the last row and column is read
        assert torch.equal(_bits(_run_pool(x, H, W, dev)), _bits(got))                # a second launch is bit-equal
        assert torch.equal(_bits(_run_pool(x, H, W, dev, extra=0)), _bits(got))       # and so is a dense output


# ---- stats ----------------------------------------------------------------------------------------------------------------------
def _stats_inputs(C, H, W, dt, pairs=1):
    """Gaussian pre-activations of a stacked batch as (2 * pairs, H, W, C) in `dt`; channel 3 non-positive in every `a` image
    and positive in every `b` image."""
    g = torch.Generator().manual_seed(C * 1000 + H * 10 + W + pairs)
    x = torch.randn(2 * pairs, H, W, C, generator=g).to(dt)
    x[:pairs, :, :, 3] = -x[:pairs, :, :, 3].abs()
    x[pairs:, :, :, 3] = x[pairs:, :, :, 3].abs() + 0.25
    return x


def _run_stats(x, pairs, H, W, dev, extra=0):
    from instantir_amd import ops
    C = x.shape[-1]
    if extra:                                           # a column slice of a wider matrix whose other columns hold NaN
        wide, xbuf = _guarded(torch.full((x.numel() // C, C + extra), float("nan"), dtype=x.dtype), dev)
        wide[:, :C] = x.reshape(-1, C).to(dev)
        xv = wide[:, :C]
    else:
        xv, xbuf = _guarded(x.reshape(-1, C), dev)
    out, obuf = _guarded(torch.full((pairs, C, 5), float("nan"), dtype=torch.float64), dev)
    ops.dists_stats(xv, pairs, H, W, out=out)
    torch.cuda.synchronize()
    assert torch.equal(_bits(xv.cpu()), _bits(x.reshape(-1, C))) and _bands_intact(obuf, out.numel())
    assert extra or _bands_intact(xbuf, x.numel())
    return out.cpu()


def _check_sums(tag, got, a, b, n):
    """`got` fp64 (N, C, 5) against the long-double sums of the fp64 features a, b (N, C, H, W), within the summation bound."""
    want, mag = R.sums(a, b)
    err = np.abs(got.numpy().astype(np.longdouble) - want)
    bound = R.sums_bound(mag, n)
    worst = float((err / np.maximum(bound, np.longdouble(1e-300))).max()) if n > 1 else 0.0
    _log(f"{tag}: max err / bound {worst:.4f} (n = {n}); max relative err {float((err / np.maximum(mag, np.longdouble(1e-300))).max()):.3e}")
    assert bool((err <= bound).all())


@pytest.mark.parametrize("name", sorted(DTYPES))
@pytest.mark.parametrize("C", [64, 128, 256, 512])
def test_stats_against_fp64(dev, C, name):
    dt = DTYPES[name]
    for H, W in SIZES:
        x = _stats_inputs(C, H, W, dt)
        f = _nchw(x)
        got = _run_stats(x, 1, H, W, dev)
        assert bool(torch.isfinite(got).all())
        _check_sums(f"stats {name} C={C} {H}x{W}", got, f[:1], f[1:], H * W)
        assert got[0, 3, [0, 2, 4]].tolist() == [0.0, 0.0, 0.0] and float(got[0, 3, 1]) > 0       # the planted channel: exactly 0
        assert torch.equal(_run_stats(x, 1, H, W, dev), got)                                      # a second launch is bit-equal
        assert torch.equal(_run_stats(x, 1, H, W, dev, extra=8), got)                             # a column slice of a wider matrix


@pytest.mark.parametrize("C,H,W", [(64, 5, 7), (512, 37, 53), (128, 1, 1)])
def test_stats_of_two_pairs_equals_two_launches(dev, C, H, W):
    """`pairs` = 2 (images a0, a1, b0, b1) gives each pair the bits of its own launch."""
    x = _stats_inputs(C, H, W, torch.float16, pairs=2)
    both = _run_stats(x, 2, H, W, dev)
    for p in range(2):
        assert torch.equal(_run_stats(x[[p, 2 + p]], 1, H, W, dev)[0], both[p])
    f = _nchw(x)
    _check_sums(f"stats pairs=2 C={C} {H}x{W}", both, f[:2], f[2:], H * W)


# ---- image_stats ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 3, 17, 23), (1, 3, 16, 16)], ids=["2x17x23", "1x16x16"])
def test_image_stats_against_fp64(dev, shape):
    from instantir_amd import ops
    N, _, H, W = shape
    rng = np.random.default_rng(3)
    u8 = [torch.from_numpy(rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)) for _ in range(2)]
    f32 = [(t.float() / 255.0).permute(0, 3, 1, 2).contiguous() for t in u8]          # the fp32 copy: u / 255 in fp32
    outs = []
    for (a, b), fill in ((u8, 255), (f32, float("nan"))):
        av, abuf = _guarded(a, dev, fill)
        bv, bbuf = _guarded(b, dev, fill)
        out, obuf = _guarded(torch.full((N, 3, 5), float("nan"), dtype=torch.float64), dev)
        ops.dists_image_stats(av, bv, out=out)
        torch.cuda.synchronize()
        assert _bands_intact(obuf, out.numel()) and torch.equal(av.cpu(), a) and torch.equal(bv.cpu(), b)
        _check_sums(f"image_stats {shape} {a.dtype}", out.cpu(), f32[0], f32[1], H * W)
        outs.append(out.cpu())
        assert torch.equal(ops.dists_image_stats(av, bv).cpu(), outs[-1])              # a second launch is bit-equal
    assert torch.equal(outs[0], outs[1])                                               # uint8 and its fp32 copy: equal bits


def test_image_stats_of_a_constant_image_cancel(dev):
    """The cancellation case: a constant 200 / 255 image has sigma^2 = 0; after the host's division the raw sums leave less than
    1e-13 (test_dists_cpu.py checks that the restatement's raw-sum form stays under the same bar)."""
    from instantir_amd import ops
    for H, W in ((16, 16), (17, 23), (512, 512)):
        u8 = torch.full((1, H, W, 3), 200, dtype=torch.uint8, device=dev)
        s = ops.dists_image_stats(u8, u8).cpu()
        n = H * W
        var = s[..., 2] / n - (s[..., 0] / n) ** 2
        cov = s[..., 4] / n - (s[..., 0] / n) * (s[..., 1] / n)
        _log(f"image_stats constant 200/255 {H}x{W}: sigma^2 {float(var.abs().max()):.3e}, sigma_ab {float(cov.abs().max()):.3e}")
        assert float(var.abs().max()) < 1e-13 and float(cov.abs().max()) < 1e-13
        assert torch.equal(s[..., 0], s[..., 1]) and torch.equal(s[..., 2], s[..., 4])


# ---- the whole network ----------------------------------------------------------------------------------------------------------
NET_SHAPES = [(2, 3, 37, 53), (1, 3, 16, 19), (1, 3, 64, 48)]
NET_SEED = 21
SMALL_WIDTHS = (8, 16, 16, 24, 8)
_NET = {}


def _net_pair(shape):
    g = torch.Generator().manual_seed(sum(shape))
    a = torch.rand(shape, generator=g)
    return a, (a + 0.1 * torch.randn(shape, generator=g)).clamp(0.0, 1.0)


def _reference(key, widths):
    """Per case the fp64 restatement, and per dtype and stage the largest e_model over the cases, the stage's two terms and both
    conv accumulation types; computed once per net."""
    if key not in _NET:
        from instantir_amd import dists as DS
        convs, alpha, beta, _, _ = DS.parse_state_dict(DS.synthetic_state_dict(NET_SEED, widths))
        ref = {"exact": [], "e_model": {name: torch.zeros(6, dtype=torch.float64) for name in DTYPES}, "weights": (convs, alpha, beta)}
        for shape in NET_SHAPES:
            a, b = _net_pair(shape)
            score, terms = R.dists(a, b, convs, alpha, beta)
            ref["exact"].append((score, terms))
            for name, dt in DTYPES.items():
                for acc in (torch.float32, torch.float64):
                    _, ts = R.dists(a, b, convs, alpha, beta, storage=dt, accumulate=acc)
                    e = (ts - terms).abs().amax(dim=(0, 2))
                    _log(f"{key} e_model {name} {shape} conv sums in {str(acc)[6:]}: " + " ".join(f"{v:.3e}" for v in e.tolist())
                         + "; score " + " ".join(f"{v:.5f}" for v in score.tolist()))
                    ref["e_model"][name] = torch.maximum(ref["e_model"][name], e)
        _NET[key] = ref
    return _NET[key]


@pytest.fixture(scope="module")
def models(dev):
    from instantir_amd.dists import DISTS
    return {name: DISTS.synthetic(NET_SEED, device=dev, dtype=dt) for name, dt in DTYPES.items()}


@pytest.mark.parametrize("name", sorted(DTYPES))
@pytest.mark.parametrize("si", range(len(NET_SHAPES)), ids=["2x37x53", "1x16x19", "1x64x48"])
def test_network_against_fp64(dev, models, si, name):
    ref = _reference("net", (64, 128, 256, 512, 512))
    model, shape = models[name], NET_SHAPES[si]
    a, b = _net_pair(shape)
    want, want_terms = ref["exact"][si]
    score, terms = model(a, b, components=True)
    torch.cuda.synchronize()
    assert score.dtype == torch.float64 and tuple(score.shape) == (shape[0],) and score.device == dev and tuple(terms.shape) == (shape[0], 6, 2)
    err = (terms.cpu() - want_terms).abs().amax(dim=(0, 2))
    bar = 3.0 * ref["e_model"][name]
    bar[0] = 1e-12                                                                     # stage 0: e_model is 0
    assert float(ref["e_model"][name][0]) == 0.0
    _log(f"net device {name} {shape}: err " + " ".join(f"{v:.3e}" for v in err.tolist()) + "; bar (3 x e_model) "
         + " ".join(f"{v:.3e}" for v in bar.tolist()) + "; err / bar " + " ".join(f"{v:.3f}" for v in (err / bar).tolist())
         + f"; score {score.cpu().tolist()} want {want.tolist()}")
    assert bool((err <= bar).all())
    assert all(float(score[n]) == float(1.0 - terms[n].sum()) for n in range(shape[0]))               # the twelve terms sum to 1 - score
    assert float((score.cpu() - (1.0 - terms.cpu().sum(dim=(1, 2)))).abs().max()) <= 1e-15
    same = model(a, a)
    _log(f"net device {name} {shape}: DISTS(a, a) = {same.cpu().tolist()}")
    assert float(same.abs().max()) <= 1e-12
    again, terms2 = model(a, b, components=True)
    assert torch.equal(again, score) and torch.equal(terms2, terms)                                  # a repeated call is bit-equal
    u8a, u8b = ((t * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous() for t in (a, b))
    fa, fb = (t.permute(0, 3, 1, 2).float() / 255 for t in (u8a, u8b))
    assert torch.equal(model(u8a, u8b), model(fa, fb)) and torch.equal(model(u8a, fb), model(fa, fb))


def test_batch_equals_single_calls(dev, models):
    model = models["fp16"]
    g = torch.Generator().manual_seed(8)
    a, b = torch.rand(3, 3, 16, 24, generator=g), torch.rand(3, 3, 16, 24, generator=g)
    score, terms = model(a, b, components=True)
    used = model.arena.buf.numel()
    for n in range(3):
        one, one_terms = model(a[n], b[n], components=True)
        assert torch.equal(one[0], score[n]) and torch.equal(one_terms[0], terms[n])
    assert model.arena.buf.numel() == used                                             # the arena does not grow with N


@pytest.mark.parametrize("name", sorted(DTYPES))
def test_weights_concentrated_on_one_stage(dev, name):
    """The wiring check the loose deep-stage bars cannot give: six models share the convs, each with alpha and beta zeroed
    outside one stage, so the score is that stage's two terms scaled by (total weight) / (the stage's weight) -- and so is the
    bar.  A slice that is off by a stage reads zero weights and scores 1."""
    from instantir_amd.dists import DISTS
    ref = _reference("small", SMALL_WIDTHS)
    convs, alpha, beta = ref["weights"]
    widths = (3,) + SMALL_WIDTHS
    a, b = _net_pair((1, 3, 16, 19))
    total, at = float(alpha.sum() + beta.sum()), 0
    for k, c in enumerate(widths):
        ak, bk = torch.zeros_like(alpha), torch.zeros_like(beta)
        ak[at:at + c], bk[at:at + c] = alpha[at:at + c], beta[at:at + c]
        at += c
        scale = total / float(ak.sum() + bk.sum())
        want, _ = R.dists(a, b, convs, ak, bk)
        got = DISTS(convs, ak, bk, device=dev, dtype=DTYPES[name])(a, b).cpu()
        bar = scale * (3.0 * float(ref["e_model"][name][k]) if k else 1e-12)
        err = float((got - want).abs().max())
        _log(f"one-stage {name} stage {k}: score {float(got[0]):.6f} want {float(want[0]):.6f} err {err:.3e} bar {bar:.3e} (scale {scale:.2f})")
        assert 0.0 < float(want[0]) < 0.9 and err <= bar


# ---- metrics and the CLI --------------------------------------------------------------------------------------------------------
def test_metrics_entry_points(dev, models):
    from PIL import Image
    from instantir_amd import metrics as M
    from instantir_amd.lpips import LPIPS
    model = models["fp16"]
    g = torch.Generator().manual_seed(8)
    a, b = torch.rand(3, 16, 24, generator=g), torch.rand(3, 16, 24, generator=g)
    ims = [Image.fromarray((t.permute(1, 2, 0) * 255).round().to(torch.uint8).numpy()) for t in (a, b)]
    one, many = M.dists(ims[0], ims[1], model), M.dists([ims[0]], [ims[1]], model)
    assert isinstance(one, float) and many == [one] and 0 < one < 1
    assert one == float(model(ims[0], ims[1])[0]) and abs(M.dists(ims[0], ims[0], model)) <= 1e-12
    plain = M.evaluate(ims[0], ims[1], device=dev)
    assert set(plain) == {"psnr", "ssim", "psnr_mean", "ssim_mean"}
    ev = M.evaluate(ims[0], ims[1], device=dev, dists_model=model)
    assert ev["dists"] == [one] and ev["dists_mean"] == one and set(ev) == set(plain) | {"dists", "dists_mean"}
    assert {k: ev[k] for k in plain} == plain
    lp = LPIPS.synthetic(6, (8, 16, 16, 24, 8), device=dev)
    both = M.evaluate(ims[0], ims[1], device=dev, lpips_model=lp, dists_model=model)
    assert set(both) == set(ev) | {"lpips", "lpips_mean"} and both["dists"] == [one]
    assert both["lpips"] == M.evaluate(ims[0], ims[1], device=dev, lpips_model=lp)["lpips"]
    big = ims[0].resize((48, 32), Image.BICUBIC)
    fid0 = M.input_fidelity(big, ims[1], device=dev)
    fid = M.input_fidelity(big, ims[1], device=dev, dists_model=model)
    assert set(fid0) == set(plain) and set(fid) == set(ev) and 0 < fid["dists"][0] < 1 and {k: fid[k] for k in fid0} == fid0
    assert set(M.input_fidelity(big, ims[1], device=dev, lpips_model=lp, dists_model=model)) == set(both)


def test_cli_dists_equals_the_python_twin(tmp_path, dev):
    from PIL import Image
    import instantir_amd.infer as cli
    from instantir_amd import dists as DS, metrics as M
    src, plain, scored = tmp_path / "clean", tmp_path / "plain", tmp_path / "scored"
    src.mkdir()
    rng = np.random.default_rng(5)
    smooth = np.kron(rng.integers(0, 255, (16, 16, 3)), np.ones((8, 8, 1))).astype(np.uint8)
    Image.fromarray(smooth).save(src / "a.png")
    weights = tmp_path / "dists.pth"
    torch.save(DS.synthetic_state_dict(6, SMALL_WIDTHS), str(weights))
    common = ["--synthetic", "tiny", "--num_inference_steps", "2", "--batch_size", "1", "--cfg", "5.0", "--test_path", str(src),
              "--degrade", "bicubic", "--degrade_seed", "3"]
    orig = cli.resize_img
    cli.resize_img = lambda im, **kw: orig(im, max_side=128, min_side=128, **kw)      # keep the tiny nets tiny
    try:
        torch.manual_seed(123)          # the VAE posterior sample draws from the global RNG
        cli.main(cli.build_parser().parse_args(common + ["--out_path", str(plain)]), dev)
        torch.manual_seed(123)
        cli.main(cli.build_parser().parse_args(common + ["--out_path", str(scored), "--dists_path", str(weights)]), dev)
    finally:
        cli.resize_img = orig
    assert (plain / "a.png").read_bytes() == (scored / "a.png").read_bytes()
    rep0, rep = json.load(open(plain / "metrics.json")), json.load(open(scored / "metrics.json"))
    assert set(rep0["files"]["a.png"]) == {"psnr", "ssim"} and set(rep0["mean"]) == {"psnr", "ssim"} and "dists" not in rep0["settings"]
    assert set(rep["files"]["a.png"]) == {"psnr", "ssim", "dists"} and rep["settings"]["dists"] == {"path": str(weights), "weights_path": None}
    assert {k: v for k, v in rep["files"]["a.png"].items() if k != "dists"} == rep0["files"]["a.png"]
    assert {k: v for k, v in rep["settings"].items() if k != "dists"} == rep0["settings"]
    twin = M.dists(Image.open(scored / "a.png").convert("RGB"), Image.open(src / "a.png").convert("RGB"), DS.DISTS.from_files(str(weights), device=dev))
    assert rep["files"]["a.png"]["dists"] == twin and rep["mean"]["dists"] == twin and 0 < twin < 1


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_on_the_device(dev, models):
    from instantir_amd.dists import DISTS, synthetic_state_dict
    model = models["fp16"]
    with pytest.raises(ValueError, match="smallest side is 16"):
        model(torch.rand(1, 3, 15, 32), torch.rand(1, 3, 15, 32))
    with pytest.raises(ValueError, match="reaches 2 GiB"):                # the size check's input mocked: nothing is allocated
        model._check_geometry(4096, 2048)
    model._check_geometry(2048, 2048)
    sd = synthetic_state_dict(2, (8, 8, 8, 8, 8))
    sd["stage2.5.weight"] = sd["stage2.5.weight"] * 3e4                    # a planted overflow: |activations| past 65504
    hot = DISTS.from_state_dict(sd, device=dev)
    a, b = _net_pair((1, 3, 16, 16))
    with pytest.raises(FloatingPointError, match="non-finite sum .* fp16; build it with dtype=torch.bfloat16"):
        hot(a, b)
    assert bool(torch.isfinite(DISTS.from_state_dict(sd, device=dev, dtype=torch.bfloat16)(a, b)).all())


def test_entries_return_einval_and_launch_nothing(dev):
    """Every refusal of the three entries with real device addresses: `ops` raises before the library is called, and the entry
    itself returns IIR_EINVAL (-1) before any HIP call.  Every call below is invalid, so none launches; the outputs keep their NaN."""
    from instantir_amd import lib, ops
    h = lib.load()
    H, W, C = 5, 7, 64
    x, _ = _guarded(torch.zeros(2 * H * W, C, dtype=torch.float16), dev)
    wide, _ = _guarded(torch.zeros(2 * H * W, C + 8, dtype=torch.float16), dev)
    pooled, _ = _guarded(torch.full((2 * 3 * 4, C), float("nan"), dtype=torch.float16), dev)
    out, _ = _guarded(torch.full((1, C, 5), float("nan"), dtype=torch.float64), dev)
    ws = torch.full((4096,), float("nan"), dtype=torch.float64, device=dev)
    xp, pp, op, wp, wb = x.data_ptr(), pooled.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel() * 8

    def pool(**k):
        a = dict(x=xp, ldx=C, images=2, H=H, W=W, C=C, dtype=0, out=pp, ldo=C)
        a.update(k)
        return h.iir_dists_l2pool(a["x"], a["ldx"], a["images"], a["H"], a["W"], a["C"], a["dtype"], a["out"], a["ldo"], None)
    for bad in (dict(x=None), dict(out=None), dict(x=xp + 8), dict(out=pp + 8), dict(images=0), dict(H=0), dict(W=0), dict(H=32769), dict(C=0),
                dict(C=12), dict(C=520), dict(ldx=56), dict(ldx=68), dict(ldo=56), dict(ldo=68), dict(dtype=2), dict(out=xp), dict(out=xp + 64)):
        assert pool(**bad) == -1, bad

    def stats(**k):
        a = dict(x=xp, ldx=C, pairs=1, H=H, W=W, C=C, dtype=0, ws=wp, ws_bytes=wb, out=op)
        a.update(k)
        return h.iir_dists_stats(a["x"], a["ldx"], a["pairs"], a["H"], a["W"], a["C"], a["dtype"], a["ws"], a["ws_bytes"], a["out"], None)
    for bad in (dict(x=None), dict(ws=None), dict(out=None), dict(pairs=0), dict(pairs=65536), dict(H=0), dict(W=40000), dict(C=0), dict(C=12),
                dict(C=520), dict(ldx=56), dict(ldx=68), dict(x=xp + 8), dict(dtype=2), dict(ws=wp + 4), dict(out=op + 4), dict(ws_bytes=C * 5 * 8 - 8)):
        assert stats(**bad) == -1, bad
    img = torch.zeros(1, 3, 16, 16, device=dev)
    ip = img.data_ptr()

    def image(**k):
        a = dict(a=ip, b=ip, u8=0, N=1, H=16, W=16, ws=wp, ws_bytes=wb, out=op)
        a.update(k)
        return h.iir_dists_image_stats(a["a"], a["b"], a["u8"], a["N"], a["H"], a["W"], a["ws"], a["ws_bytes"], a["out"], None)
    for bad in (dict(a=None), dict(b=None), dict(ws=None), dict(out=None), dict(N=0), dict(N=65536), dict(H=0), dict(W=32769), dict(a=ip + 2),
                dict(b=ip + 1), dict(ws=wp + 4), dict(out=op + 4), dict(ws_bytes=3 * 5 * 8 - 8)):
        assert image(**bad) == -1, bad
    # through ops: the same refusals as ValueError, before the library is called
    for kw, msg in ((dict(x=x[:69]), "x must be"), (dict(x=wide[:, 1:65]), "x must be|aligned"), (dict(out=pooled[:23]), "out must be"),
                    (dict(out=x[:24]), "overlaps x"), (dict(out=pooled.bfloat16()), "x's dtype"), (dict(H=0), "H must be")):
        args = dict(x=x, images=2, H=H, W=W, out=pooled)
        args.update(kw)
        with pytest.raises(ValueError, match="dists_l2pool: .*(" + msg + ")"):
            ops.dists_l2pool(**args)
    for kw, msg in ((dict(x=x[:69]), "x must be"), (dict(pairs=0), "pairs must be"), (dict(out=out[:, :32]), "out must be"),
                    (dict(ws=ws[:8]), "ws needs"), (dict(ws=ws.cpu()), "ws needs")):
        args = dict(x=x, pairs=1, H=H, W=W, ws=ws, out=out)
        args.update(kw)
        with pytest.raises(ValueError, match="dists_stats: .*" + msg):
            ops.dists_stats(**args)
    for kw, msg in ((dict(b=img[:, :, :, :15].contiguous()), "share a dtype and a shape"), (dict(b=img.cpu()), "CUDA"),
                    (dict(out=out), "out must be"), (dict(ws=ws[:2]), "ws needs")):
        args = dict(a=img, b=img.clone(), ws=ws)
        args.update(kw)
        with pytest.raises(ValueError, match="dists_image_stats: .*" + msg):
            ops.dists_image_stats(**args)
    torch.cuda.synchronize()
    assert bool(torch.isnan(pooled).all()) and bool(torch.isnan(out).all()) and bool(torch.isnan(ws).all())     # nothing was launched
