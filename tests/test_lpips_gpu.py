"""GPU: the LPIPS kernels (ops.lpips_prep / relu_ / lpips_tap), the whole network (instantir_amd.lpips.LPIPS) and the CLI wiring
against the fp64 restatement of the contract (tests/lpips_ref.py).

Bounds (from the contract and the rounding points, DESIGN.md section 7 "LPIPS", not from what the kernels give):
  prep:  |kernel - fp64| <= one rounding of the 16-bit type (2^-11 or 2^-8 relative) + 2^-22: the affine runs in fp64 on the fp32
         pixel value, so what is left is the rounding to fp32 and to the 16-bit type; pad channels exactly 0; a uint8 image and its
         fp32 copy give equal bits.
  relu:  exact.
  tap:   on the same 16-bit pre-activations, with u = 2^-24 (lpips_ref.tap_bounds, where the derivation stands):
         |err d(p)| <= max_w u (8 C + 44) per pixel of the map, |err D| <= max_w u (8 C + 56); the pooled output is exact (max and
         ReLU commute, and it is a selection).  The measured error is a small fraction of the bound (the sums are trees over lanes,
         the bound is for any order), so a slip of one pixel is caught by the map, which is compared pixel by pixel.
  net:   |D_l - fp64| <= 3 x the largest e_model of that dtype and layer over the cases, e_model = |restatement(storage = dtype)
         - restatement(fp64)| measured on the CPU (the factor 3: another fp32 summation order inside the MFMA tiles).
Every figure is printed before its assertion (run with -s to keep them; profiles/lpips_test_figures.log is such a run).
Every operand lies inside a larger buffer filled with NaN."""
import json

import numpy as np
import pytest
import torch

import lpips_ref as R

pytestmark = pytest.mark.gpu

PAD = 4096
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}


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


# ---- prep -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(DTYPES))
@pytest.mark.parametrize("shape", [(2, 3, 17, 23), (1, 3, 16, 16)], ids=["2x17x23", "1x16x16"])
def test_prep_against_fp64(dev, shape, name):
    from instantir_amd import ops
    dt = DTYPES[name]
    N, _, H, W = shape
    u8 = torch.from_numpy(np.random.default_rng(3).integers(0, 255, (N, H, W, 3), dtype=np.uint8))
    u8[0, 0, 0] = torch.tensor([0, 254, 128], dtype=torch.uint8)
    f32 = (u8.float() / 255.0).permute(0, 3, 1, 2).contiguous()                   # the fp32 copy: u / 255 in fp32
    want = R.prep(f32).permute(0, 2, 3, 1).reshape(N * H * W, 3)
    outs = []
    for src, fill in ((u8, 255), (f32, float("nan"))):
        s, _ = _guarded(src, dev, fill)
        out, buf = _guarded(torch.full((N * H * W, ops.LPIPS_CPAD), float("nan"), dtype=dt), dev)
        ops.lpips_prep(s, out)
        torch.cuda.synchronize()
        assert _bands_intact(buf, out.numel())
        assert bool((out[:, 3:] == 0).all())                                       # pad channels exactly 0
        got = out[:, :3].double().cpu()
        err = (got - want).abs()
        bound = R.ROUNDING[dt] * want.abs() + 2.0 ** -22
        _log(f"prep {name} {shape} {src.dtype}: max err / bound {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all())
        outs.append(out.clone())
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))       # uint8 and fp32 sources bit-equal
    # a wider row stride: the columns past CPAD keep their bits
    wide, _ = _guarded(torch.full((N * H * W, 72), 7.0, dtype=dt), dev)
    ops.lpips_prep(_guarded(f32, dev)[0], wide)
    assert torch.equal(wide[:, :64].view(torch.int16), outs[1].view(torch.int16)) and bool((wide[:, 64:] == 7.0).all())


# ---- relu -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(DTYPES))
@pytest.mark.parametrize("rows,C", [(391, 64), (1, 512)])
def test_relu_is_exact(dev, rows, C, name):
    from instantir_amd import ops
    dt = DTYPES[name]
    g = torch.Generator().manual_seed(rows)
    x = (torch.randn(rows, C, generator=g) * 3).to(dt)
    x[0, :4] = torch.tensor([float("-inf"), float("inf"), -0.0, 0.0], dtype=dt)
    x[-1, -1] = float("nan")
    view, buf = _guarded(x, dev)
    ops.relu_(view)
    torch.cuda.synchronize()
    assert _bands_intact(buf, x.numel())
    want = torch.where(x < 0, torch.zeros_like(x), x)
    got = view.cpu()
    assert bool(torch.isnan(got[-1, -1])) and float(got[0, 0]) == 0.0 and float(got[0, 1]) == float("inf")
    keep = ~torch.isnan(want)
    assert torch.equal(got[keep], want[keep]) and not bool(torch.signbit(got[keep]).any())
    # a column slice of a wider matrix: the other columns keep their bits
    wide, _ = _guarded(torch.full((rows, C + 8), -2.0, dtype=dt), dev)
    wide[:, :C].copy_(x)
    ops.relu_(wide[:, :C])
    assert bool((wide[:, C:] == -2.0).all()) and torch.equal(wide[:, :C].cpu()[keep], want[keep])


# ---- tap ------------------------------------------------------------------------------------------------------------------------
TAP_SIZES = [(5, 7), (16, 16), (37, 53)]


def _tap_inputs(C, H, W, dt, pairs=1):
    """Gaussian pre-activations (about half negative) of a stacked batch as (2 * pairs, H, W, C) in `dt`, with planted pixels
    whose channels are all non-positive in a only, b only and both; lin weights in [0, 1)."""
    g = torch.Generator().manual_seed(C * 1000 + H * 10 + W)
    x = torch.randn(2 * pairs, H, W, C, generator=g).to(dt)
    x[0, 1, 2] = -x[0, 1, 2].abs()                       # a only
    x[pairs, 2, 3] = -x[pairs, 2, 3].abs()               # b only
    x[0, 3, 4] = -x[0, 3, 4].abs()                       # both
    x[pairs, 3, 4] = 0.0
    x[0, H - 1, W - 1, 0] = 3.0                          # the last pixel, which an odd size scores and does not pool
    return x, torch.rand(C, generator=g)


def _run_tap(x, lin, pairs, H, W, dev, pooled=True, dmap=True):
    from instantir_amd import ops
    C = x.shape[-1]
    xv, xbuf = _guarded(x.reshape(-1, C), dev)
    pv = pbuf = dv = dbuf = None
    if pooled:
        pv, pbuf = _guarded(torch.full((2 * pairs * (H // 2) * (W // 2), C), float("nan"), dtype=x.dtype), dev)
    if dmap:
        dv, dbuf = _guarded(torch.full((pairs, H, W), float("nan")), dev)
    D = ops.lpips_tap(xv, pairs, H, W, lin.to(dev), pooled=pv, dmap=dv)
    torch.cuda.synchronize()
    assert torch.equal(xv.cpu().view(torch.int16), x.reshape(-1, C).view(torch.int16)) and _bands_intact(xbuf, x.numel())
    assert pbuf is None or _bands_intact(pbuf, pv.numel())
    assert dbuf is None or _bands_intact(dbuf, dv.numel())
    return D.cpu(), None if pv is None else pv.cpu(), None if dv is None else dv.cpu()


@pytest.mark.parametrize("name", sorted(DTYPES))
@pytest.mark.parametrize("C", [64, 128, 256, 512])
def test_tap_against_fp64(dev, C, name):
    dt = DTYPES[name]
    for H, W in TAP_SIZES:
        x, lin = _tap_inputs(C, H, W, dt)
        nchw = x.double().permute(0, 3, 1, 2)
        d_ref, D_ref, pa, pb = R.tap(nchw[:1], nchw[1:], lin)
        assert float(d_ref[0, 3, 4]) == 0.0 and float(d_ref[0, 1, 2]) > 0 and float(d_ref[0, 2, 3]) > 0      # the planted pixels
        D, pooled, dmap = _run_tap(x, lin, 1, H, W, dev)
        bound_d, bound_D = R.tap_bounds(C, float(lin.max()))
        err_d, err_D = float((dmap.double() - d_ref).abs().max()), float((D - D_ref).abs().max())
        _log(f"tap {name} C={C} {H}x{W}: map err {err_d:.3e} / bound {bound_d:.3e} = {err_d / bound_d:.4f}; "
             f"D err {err_D:.3e} / bound {bound_D:.3e} = {err_D / bound_D:.4f}; D = {float(D_ref[0]):.6f}")
        assert bool(torch.isfinite(dmap).all()) and float(dmap[0, 3, 4]) == 0.0
        assert err_d <= bound_d and err_D <= bound_D
        want_pool = torch.cat([pa, pb]).permute(0, 2, 3, 1).reshape(-1, C)
        assert torch.equal(pooled.double(), want_pool)                                 # exact: a selection
        # without the optional outputs: the same bits; and a second launch
        D2, _, _ = _run_tap(x, lin, 1, H, W, dev, pooled=False, dmap=False)
        D3, pooled3, dmap3 = _run_tap(x, lin, 1, H, W, dev)
        assert torch.equal(D2, D) and torch.equal(D3, D) and torch.equal(dmap3, dmap)
        assert torch.equal(pooled3.view(torch.int16), pooled.view(torch.int16))


def test_tap_of_two_pairs_equals_two_taps(dev):
    """`pairs` = 2 (images a0, a1, b0, b1) gives each pair the bits of its own launch; 1 x 1 has no quad to pool."""
    H, W, C = 5, 7, 64
    x, lin = _tap_inputs(C, H, W, torch.float16, pairs=2)
    D, pooled, dmap = _run_tap(x, lin, 2, H, W, dev)
    q = (H // 2) * (W // 2)
    for p in range(2):
        D1, pooled1, dmap1 = _run_tap(x[[p, 2 + p]], lin, 1, H, W, dev)
        assert torch.equal(D1[0], D[p]) and torch.equal(dmap1[0], dmap[p])
        assert torch.equal(pooled1[:q], pooled[p * q:(p + 1) * q]) and torch.equal(pooled1[q:], pooled[(2 + p) * q:(3 + p) * q])
    x1, lin1 = torch.randn(2, 1, 1, 512, generator=torch.Generator().manual_seed(4)).half(), torch.rand(512)
    D1, _, dmap1 = _run_tap(x1, lin1, 1, 1, 1, dev, pooled=False)
    d_ref, D_ref, _, _ = R.tap(x1[:1].double().permute(0, 3, 1, 2), x1[1:].double().permute(0, 3, 1, 2), lin1)
    assert abs(float(D1[0]) - float(D_ref[0])) <= R.tap_bounds(512, 1.0)[1]


# ---- the whole network ----------------------------------------------------------------------------------------------------------
NET_SHAPES = [(2, 3, 37, 53), (1, 3, 16, 19), (1, 3, 64, 48)]
NET_SEED = 21
_NET = {}


def _net_pair(shape):
    g = torch.Generator().manual_seed(sum(shape))
    a = torch.rand(shape, generator=g)
    return a, (a + 0.1 * torch.randn(shape, generator=g)).clamp(0.0, 1.0)


def _net_reference():
    """Per case the fp64 restatement, and per dtype and layer the largest e_model over the cases; computed once."""
    if not _NET:
        from instantir_amd import lpips as LP
        convs, lins, _, _ = LP.parse_state_dict(LP.synthetic_state_dict(NET_SEED))
        _NET["exact"] = []
        e_model = {name: torch.zeros(5, dtype=torch.float64) for name in DTYPES}
        for shape in NET_SHAPES:
            a, b = _net_pair(shape)
            D, maps = R.lpips(a, b, convs, lins)
            _NET["exact"].append((D, maps))
            for name, dt in DTYPES.items():
                Ds, _ = R.lpips(a, b, convs, lins, storage=dt)
                e = (Ds - D).abs().max(dim=0).values
                _log(f"net e_model {name} {shape}: " + " ".join(f"{v:.3e}" for v in e.tolist()) + "; D = "
                     + " ".join(f"{v:.5f}" for v in D[0].tolist()))
                e_model[name] = torch.maximum(e_model[name], e)
        _NET["e_model"] = e_model
    return _NET


@pytest.fixture(scope="module")
def models(dev):
    from instantir_amd.lpips import LPIPS
    return {name: LPIPS.synthetic(NET_SEED, device=dev, dtype=dt) for name, dt in DTYPES.items()}


@pytest.mark.parametrize("name", sorted(DTYPES))
@pytest.mark.parametrize("si", range(len(NET_SHAPES)), ids=["2x37x53", "1x16x19", "1x64x48"])
def test_network_against_fp64(dev, models, si, name):
    ref = _net_reference()
    model, shape = models[name], NET_SHAPES[si]
    a, b = _net_pair(shape)
    want, want_maps = ref["exact"][si]
    (D, maps) = model(a, b, layers=True, spatial=True)
    total = model(a, b)
    torch.cuda.synchronize()
    assert D.dtype == torch.float64 and tuple(D.shape) == (shape[0], 5) and D.device == dev and tuple(total.shape) == (shape[0],)
    err = (D.cpu() - want).abs().max(dim=0).values
    bar = 3.0 * ref["e_model"][name]
    _log(f"net device {name} {shape}: err " + " ".join(f"{v:.3e}" for v in err.tolist()) + "; bar (3 x e_model) "
         + " ".join(f"{v:.3e}" for v in bar.tolist()))
    assert bool((err <= bar).all())
    assert torch.equal(total, D.sum(dim=1))                                            # layers=True sums to the total
    assert [tuple(m.shape) for m in maps] == [tuple(m.shape) for m in want_maps] and all(m.dtype == torch.float32 for m in maps)
    for l, m in enumerate(maps):
        assert float((m.double().mean(dim=(1, 2)).cpu() - D[:, l].cpu()).abs().max()) <= 1e-6 * (1 + float(D[:, l].max()))
    assert torch.equal(model(a, a), torch.zeros(shape[0], dtype=torch.float64, device=dev))            # exactly 0.0
    assert torch.equal(model(a, b, layers=True), D)                                    # a repeated call is bit-equal
    u8a, u8b = ((t * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous() for t in (a, b))
    assert torch.equal(model(u8a, u8b), model(u8a.permute(0, 3, 1, 2).float() / 255, u8b.permute(0, 3, 1, 2).float() / 255))


def test_batch_equals_single_calls(dev, models):
    model = models["fp16"]
    g = torch.Generator().manual_seed(8)
    a, b = torch.rand(3, 3, 16, 24, generator=g), torch.rand(3, 3, 16, 24, generator=g)
    D = model(a, b, layers=True)
    used = model.arena.buf.numel()
    for n in range(3):
        assert torch.equal(model(a[n], b[n], layers=True)[0], D[n])
    assert model.arena.buf.numel() == used                                             # the arena does not grow with N
    from instantir_amd import metrics as M
    from PIL import Image
    ims = [Image.fromarray((t.permute(1, 2, 0) * 255).round().to(torch.uint8).numpy()) for t in (a[0], b[0])]
    one, many = M.lpips(ims[0], ims[1], model), M.lpips([ims[0]], [ims[1]], model)
    assert isinstance(one, float) and many == [one] and one > 0
    ev = M.evaluate(ims[0], ims[1], device=dev, lpips_model=model)
    assert ev["lpips"] == [one] and ev["lpips_mean"] == one and set(ev) == {"psnr", "ssim", "lpips", "psnr_mean", "ssim_mean", "lpips_mean"}
    assert set(M.evaluate(ims[0], ims[1], device=dev)) == {"psnr", "ssim", "psnr_mean", "ssim_mean"}
    big = ims[0].resize((48, 32), Image.BICUBIC)
    fid = M.input_fidelity(big, ims[1], device=dev, lpips_model=model)
    assert set(fid) == set(ev) and fid["lpips"][0] > 0


def test_refusals_on_the_device(dev, models):
    from instantir_amd.lpips import LPIPS, parse_state_dict, synthetic_state_dict
    model = models["fp16"]
    with pytest.raises(ValueError, match="smallest side is 16"):
        model(torch.rand(1, 3, 15, 32), torch.rand(1, 3, 15, 32))
    with pytest.raises(ValueError, match="reaches 2 GiB"):                # the size check's input mocked: nothing is allocated
        model._check_geometry(4096, 2048)
    model._check_geometry(2048, 2048)
    sd = synthetic_state_dict(2, (8, 8, 8, 8, 8))
    sd["net.slice2.5.weight"] = sd["net.slice2.5.weight"] * 3e4          # a planted overflow: |activations| past 65504
    hot = LPIPS.from_state_dict(sd, device=dev)
    a, b = _net_pair((1, 3, 16, 16))
    with pytest.raises(FloatingPointError, match="non-finite tap .* fp16"):
        hot(a, b)
    assert bool(torch.isfinite(LPIPS.from_state_dict(sd, device=dev, dtype=torch.bfloat16)(a, b)).all())


# ---- the CLI --------------------------------------------------------------------------------------------------------------------
def test_cli_lpips_equals_the_python_twin(tmp_path, dev):
    from PIL import Image
    import instantir_amd.infer as cli
    from instantir_amd import lpips as LP, metrics as M
    src, plain, scored = tmp_path / "clean", tmp_path / "plain", tmp_path / "scored"
    src.mkdir()
    rng = np.random.default_rng(5)
    smooth = np.kron(rng.integers(0, 255, (16, 16, 3)), np.ones((8, 8, 1))).astype(np.uint8)
    Image.fromarray(smooth).save(src / "a.png")
    weights = tmp_path / "lpips.pth"
    torch.save(LP.synthetic_state_dict(6, (8, 16, 16, 24, 8)), str(weights))
    common = ["--synthetic", "tiny", "--num_inference_steps", "2", "--batch_size", "1", "--cfg", "5.0", "--test_path", str(src),
              "--degrade", "bicubic", "--degrade_seed", "3"]
    orig = cli.resize_img
    cli.resize_img = lambda im, **kw: orig(im, max_side=128, min_side=128, **kw)      # keep the tiny nets tiny
    try:
        torch.manual_seed(123)          # the VAE posterior sample draws from the global RNG
        cli.main(cli.build_parser().parse_args(common + ["--out_path", str(plain)]), dev)
        torch.manual_seed(123)
        cli.main(cli.build_parser().parse_args(common + ["--out_path", str(scored), "--lpips_path", str(weights)]), dev)
    finally:
        cli.resize_img = orig
    assert (plain / "a.png").read_bytes() == (scored / "a.png").read_bytes()
    rep0, rep = json.load(open(plain / "metrics.json")), json.load(open(scored / "metrics.json"))
    assert set(rep0["files"]["a.png"]) == {"psnr", "ssim"} and set(rep0["mean"]) == {"psnr", "ssim"} and "lpips" not in rep0["settings"]
    assert set(rep["files"]["a.png"]) == {"psnr", "ssim", "lpips"} and rep["settings"]["lpips"] == {"path": str(weights), "lin_path": None}
    assert {k: v for k, v in rep["files"]["a.png"].items() if k != "lpips"} == rep0["files"]["a.png"]
    twin = M.lpips(Image.open(scored / "a.png").convert("RGB"), Image.open(src / "a.png").convert("RGB"), LP.LPIPS.from_files(str(weights), device=dev))
    assert rep["files"]["a.png"]["lpips"] == twin and rep["mean"]["lpips"] == twin and twin > 0
