"""CPU: FreeU (module/min_sdxl.py:22-77) -- the fp32 restatement the GPU tests use as their oracle, pinned to the reference's
own outputs (tests/golden/freeu.npz, tests/golden/make_freeu_golden.py); the closed form the HIP kernels evaluate; argument
validation of the new C entries (before any HIP call, so no GPU is needed); the pipeline / CLI switches as host logic."""
import math
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "freeu.npz")
SHAPES = [(32, 32), (64, 64), (24, 32), (5, 7), (2, 2), (1, 4)]


# ---- the fp32 restatement (torch.fft), shared with tests/test_freeu_gpu.py -----------------------------------------------
def fourier_filter(x, s):
    """fourier_filter(x, threshold=1, scale=s) of module/min_sdxl.py:22-48, in fp32 for every size."""
    x = x.float()
    H, W = x.shape[-2:]
    X = torch.fft.fftshift(torch.fft.fftn(x, dim=(-2, -1)), dim=(-2, -1))
    mask = torch.ones(H, W)
    crow, ccol = H // 2, W // 2
    mask[crow - 1:crow + 1, ccol - 1:ccol + 1] = s
    X = X * mask.to(X.device)
    return torch.fft.ifftn(torch.fft.ifftshift(X, dim=(-2, -1)), dim=(-2, -1)).real


def apply_freeu(idx, hidden, skip, factors):
    """apply_freeu of module/min_sdxl.py:51-77 on NCHW fp32 tensors; factors = (s1, s2, b1, b2).  Returns new tensors."""
    hidden, skip = hidden.float().clone(), skip.float()
    if idx not in (0, 1):
        return hidden, skip
    s, b = factors[idx], factors[2 + idx]
    half = hidden.shape[1] // 2
    hidden[:, :half] = hidden[:, :half] * b
    return hidden, fourier_filter(skip, s)


def closed_form(v, s):
    """The rank-<=4 correction the HIP kernels evaluate (csrc/freeu.hip), in fp64 from exact integer phases."""
    v = np.asarray(v, dtype=np.float64)
    H, W = v.shape[-2:]
    h = np.arange(H)[:, None]
    w = np.arange(W)[None, :]
    freqs = [(0, 0)] + ([(1, 0)] if H > 1 else []) + ([(0, 1)] if W > 1 else []) + ([(1, 1)] if H > 1 and W > 1 else [])
    corr = np.zeros_like(v)
    for a, b in freqs:
        n = (a * h * W + b * w * H) % (H * W)
        phi = 2 * math.pi * n / (H * W)
        c, sn = np.cos(phi), np.sin(phi)
        C = (v * c).sum(axis=(-2, -1), keepdims=True)
        S = (v * sn).sum(axis=(-2, -1), keepdims=True)
        corr += C * c + S * sn
    return v + (s - 1.0) / (H * W) * corr


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("H,W", SHAPES)
def test_restatement_matches_reference_golden(golden, H, W):
    f = tuple(golden["factors"].tolist())
    tag = f"{H}x{W}"
    hidden = torch.from_numpy(golden[f"{tag}.hidden"]).float()
    skip = torch.from_numpy(golden[f"{tag}.skip"]).float()
    for idx in (0, 1):
        h, s = apply_freeu(idx, hidden, skip, f)
        assert (h - torch.from_numpy(golden[f"{tag}.hidden_out{idx}"])).abs().max().item() <= 1e-5
        assert (s - torch.from_numpy(golden[f"{tag}.skip_out{idx}"])).abs().max().item() <= 1e-5
        # and the reference really filtered: the skip moved
        assert not torch.allclose(s, skip, atol=1e-3) or (H, W) == (1, 1)


@pytest.mark.parametrize("H,W", SHAPES + [(3, 1), (1, 1), (3, 5)])
def test_closed_form_equals_fft_filter(golden, H, W):
    """The 7-sum closed form (frequencies {0, -1} x {0, -1}, the DIAGONAL (1, 1), duplicates dropped for H or W == 1) against
    the fp64 FFT filter, and against the reference's golden where one exists."""
    g = torch.Generator().manual_seed(H * 100 + W)
    v = torch.randn(2, 3, H, W, generator=g, dtype=torch.float64)
    for s in (0.9, 0.2, 1.7):
        X = torch.fft.fftshift(torch.fft.fftn(v, dim=(-2, -1)), dim=(-2, -1))
        mask = torch.ones(H, W, dtype=torch.float64)
        mask[H // 2 - 1:H // 2 + 1, W // 2 - 1:W // 2 + 1] = s
        want = torch.fft.ifftn(torch.fft.ifftshift(X * mask, dim=(-2, -1)), dim=(-2, -1)).real.numpy()
        assert np.abs(closed_form(v.numpy(), s) - want).max() <= 1e-12
    tag = f"{H}x{W}"
    if f"{tag}.skip" in golden.files:
        f = golden["factors"]
        for idx in (0, 1):
            got = closed_form(golden[f"{tag}.skip"].astype(np.float64), float(f[idx]))
            assert np.abs(got - golden[f"{tag}.skip_out{idx}"]).max() <= 1e-5


# ---- C ABI: every precondition is refused with IIR_EINVAL before any HIP call -----------------------------------------
def test_partials_size_query():
    from instantir_amd import lib
    h = lib.load()
    assert h.iir_freeu_partials_bytes(2 * 32 * 32, 32, 32, 1280) == 2 * 16 * 7 * 1280 * 4
    assert h.iir_freeu_partials_bytes(2 * 24 * 32, 24, 32, 640) == 2 * 16 * 7 * 640 * 4
    assert h.iir_freeu_partials_bytes(100, 32, 32, 1280) == -1        # rows not whole images
    assert h.iir_freeu_partials_bytes(1024, 32, 32, 1276) == -1       # C % 8
    assert h.iir_freeu_partials_bytes(16, 0, 4, 64) == -1             # H < 1


def test_freeu_stats_rejects_bad_arguments_without_a_gpu():
    from instantir_amd import lib
    h = lib.load()
    P = 4096
    rows, H, W, C = 2 * 8 * 8, 8, 8, 64
    nb = h.iir_freeu_partials_bytes(rows, H, W, C)

    def call(**kw):
        a = dict(skip=P, lds=C, add=None, lda=0, scale=None, rows=rows, H=H, W=W, C=C, part=P, nb=nb)
        a.update(kw)
        return h.iir_freeu_stats_f16(a["skip"], a["lds"], a["add"], a["lda"], a["scale"], a["rows"], a["H"], a["W"], a["C"],
                                     a["part"], a["nb"], None)

    assert call(skip=None) == -1
    assert call(part=None) == -1
    assert call(C=60) == -1                      # C % 8
    assert call(C=0) == -1
    assert call(lds=68) == -1                    # stride % 8
    assert call(lds=56) == -1                    # stride < C
    assert call(add=P, lda=12) == -1             # add stride % 8
    assert call(rows=rows + 8) == -1             # rows % (H W)
    assert call(H=0) == -1 and call(W=0) == -1
    assert call(nb=nb - 4) == -1                 # partials too small


def test_freeu_concat_rejects_bad_arguments_without_a_gpu():
    from instantir_amd import lib
    h = lib.load()
    P = 4096
    rows, H, W, cx, cs = 2 * 4 * 4, 4, 4, 256, 128
    nb = h.iir_freeu_partials_bytes(rows, H, W, cs)

    def call(**kw):
        a = dict(x=P, ldx=cx, cx=cx, mid=None, ldm=0, sk=P, lds=cs, cs=cs, add=None, lda=0, scale=None, rows=rows, H=H, W=W,
                 part=P, nb=nb, cat=P, ldc=cx + cs, off=0)
        a.update(kw)
        return h.iir_freeu_concat_f16(a["x"], a["ldx"], a["cx"], a["mid"], a["ldm"], a["sk"], a["lds"], a["cs"], a["add"], a["lda"],
                                      a["scale"], a["rows"], a["H"], a["W"], 1.3, 0.9, a["part"], a["nb"], a["cat"], a["ldc"],
                                      a["off"], None)

    for k in ("x", "sk", "cat", "part"):
        assert call(**{k: None}) == -1, k
    assert call(cx=252) == -1 and call(cs=124) == -1 and call(cx=0) == -1 and call(cs=0) == -1
    assert call(ldx=260) == -1 and call(ldx=248) == -1
    assert call(lds=132) == -1 and call(lds=120) == -1
    assert call(mid=P, ldm=4) == -1 and call(mid=P, ldm=248) == -1
    assert call(add=P, lda=4) == -1 and call(add=P, lda=120) == -1
    assert call(ldc=cx + cs - 8) == -1                       # concat does not fit the row
    assert call(off=8) == -1                                 # ... with the offset
    assert call(off=4, ldc=cx + cs + 8) == -1                # offset % 8
    assert call(off=-8, ldc=cx + cs + 8) == -1
    assert call(ldc=cx + cs + 4) == -1                       # ldc % 8
    assert call(rows=rows - 1) == -1 and call(H=0) == -1
    assert call(nb=nb - 4) == -1


# ---- host logic: pipeline switch, shared state, zero gate, CLI ----------------------------------------------------------
def _pipe():
    from instantir_amd.config import UNetConfig
    from instantir_amd.pipeline import InstantIRPipeline
    return InstantIRPipeline(UNetConfig.tiny(), {}, device="cpu")


def test_enable_disable_and_shared_state():
    p = _pipe()
    assert p._freeu is None
    p.enable_freeu(0.9, 0.2, 1.3, 1.4)
    assert p._freeu == (0.9, 0.2, 1.3, 1.4)
    p.unet.disable_freeu()                       # diffusers' unet-level switch: same state
    assert p._freeu is None
    p.unet.enable_freeu(1, 1, 1, 1)
    assert p._freeu == (1.0, 1.0, 1.0, 1.0)
    p.disable_freeu()
    assert p._freeu is None


@pytest.mark.parametrize("factors", [(0, 0.2, 1.3, 1.4), (0.9, 0.0, 1.3, 1.4), (0.9, 0.2, 0, 1.4), (0.9, 0.2, 1.3, 0.0)])
def test_any_zero_factor_disables_freeu(factors):
    """`s1 and s2 and b1 and b2` (module/unet/unet_2d_ZeroSFT_blocks.py:2600-2605): one zero switches it off everywhere."""
    p = _pipe()
    p.enable_freeu(0.9, 0.2, 1.3, 1.4)
    p.enable_freeu(*factors)
    assert p._freeu is None


def test_setting_reaches_every_unet():
    class Net:
        freeu = None
    p = _pipe()
    a, b = Net(), Net()
    p.enable_freeu(0.9, 0.2, 1.3, 1.4)
    p._apply_freeu(a, None, b)
    assert a.freeu == b.freeu == (0.9, 0.2, 1.3, 1.4)
    p.disable_freeu()
    p._apply_freeu(a, b)
    assert a.freeu is None and b.freeu is None


def test_cli_freeu_flag():
    from instantir_amd.infer import apply_freeu, build_parser
    args = build_parser().parse_args(["--test_path", "x", "--freeu", "0.9", "0.2", "1.3", "1.4"])
    assert args.freeu == [0.9, 0.2, 1.3, 1.4]
    p = _pipe()
    apply_freeu(p, args)
    assert p._freeu == (0.9, 0.2, 1.3, 1.4)
    off = build_parser().parse_args(["--test_path", "x"])
    assert off.freeu is None
    p2 = _pipe()
    apply_freeu(p2, off)
    assert p2._freeu is None
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--test_path", "x", "--freeu", "0.9", "0.2", "1.3"])
