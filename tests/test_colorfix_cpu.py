"""CPU: LQ-guided colour fix (color_fix: wavelet, adain) -- the contract's two forms agree, the ABI entries exist and reject
bad arguments before any HIP call, the CLI flag, and the pipeline refusals that need no device."""
import ctypes as C

import pytest
import torch

import colorfix_ref as R
from instantir_amd import lib
from instantir_amd.config import UNetConfig

NEW = ("iir_colorfix_workspace_bytes", "iir_colorfix_wavelet_f32", "iir_colorfix_adain_f32")


# ---- the contract ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(5, 7), (8, 8), (24, 40), (257, 131)])
def test_textbook_and_difference_forms_agree_in_fp64(H, W):
    """decompose(content).high + decompose(style).low == content + B(style - content), B separable with per-level index clamps
    (also where a side is shorter than the dilation)."""
    c, s = R.recipe(2, H, W, 3)
    c, s = c.double(), s.double()
    a, b = R.wavelet(c, s), R.wavelet_difference(c, s)
    assert (a - b).abs().max().item() <= 1e-12
    # before the clamp too (the clamp could hide a difference)
    hi, lo = R.decompose(c)[0], R.decompose(s)[1]
    d = s - c
    for r in R.LEVELS:
        d = R._tap(d, r, 3)
    for r in R.LEVELS:
        d = R._tap(d, r, 2)
    assert ((hi + lo) - (c + d)).abs().max().item() <= 1e-12


def test_per_level_clamp_differs_from_one_edge_extension():
    """What the kernel's halo must reproduce: clamping the index at every level is not one replicate extension by 31."""
    c, s = R.recipe(1, 8, 8, 5)
    d = (s - c).double()
    per_level = d
    for r in R.LEVELS:
        per_level = R._tap(per_level, r, 2)
    i = torch.arange(-31, 8 + 31).clamp(0, 7)
    ext = d[:, :, i]
    for r in R.LEVELS:
        n = ext.shape[2]
        j = torch.arange(n)
        ext = 0.25 * ext[:, :, (j - r).clamp(0, n - 1)] + 0.25 * ext[:, :, (j + r).clamp(0, n - 1)] + 0.5 * ext
    assert (ext[:, :, 31:39] - per_level).abs().max().item() > 1e-3


@pytest.mark.parametrize("H,W", [(5, 7), (24, 40)])
def test_identities(H, W):
    g = torch.Generator().manual_seed(1)
    c = (0.1 + 0.6 * torch.rand(2, 3, H, W, generator=g)).double()
    assert (R.wavelet(c, c) - c).abs().max().item() <= 1e-12                  # style == content returns content
    assert (R.wavelet(c, c + 0.25) - (c + 0.25)).abs().max().item() <= 1e-12  # a constant offset is transferred whole
    assert (R.adain(c, c) - c).abs().max().item() <= 1e-12
    with pytest.raises(ValueError):
        R.adain(c[:, :, :1, :1], c[:, :, :1, :1])


# ---- ABI ------------------------------------------------------------------------------------------------------------------
def test_new_entries_are_declared_bound_and_exported():
    syms = lib.declared_symbols()
    for name in NEW:
        assert name in syms and name in lib.SIGNATURES
    assert sorted(syms) == sorted(lib.SIGNATURES)
    h = C.CDLL(lib.LIB_PATH)
    for name in NEW:
        assert hasattr(h, name), name
    assert lib.load().iir_abi_version() == 3


def test_workspace_bytes():
    h = lib.load()
    assert h.iir_colorfix_workspace_bytes(1, 3, 1024, 1024) == 3 * 1024 * 1024 * 4      # one plane set
    assert h.iir_colorfix_workspace_bytes(2, 3, 5, 7) == 2 * 6 * 64 * 3 * 4             # the slab table is larger
    for bad in ((0, 3, 8, 8), (1, 0, 8, 8), (1, 3, 0, 8), (1, 3, 8, -1), (1, 3, 40000, 8)):
        assert h.iir_colorfix_workspace_bytes(*bad) == -1, bad


@pytest.mark.parametrize("name", NEW[1:])
def test_bad_arguments_are_rejected_without_a_gpu(name):
    h = lib.load()
    fn = getattr(h, name)
    P = 4096
    need = h.iir_colorfix_workspace_bytes(1, 3, 8, 8)

    def call(**kw):
        a = dict(content=P, style=P, out=P, B=1, C=3, H=8, W=8, ws=P, ws_bytes=need)
        a.update(kw)
        return fn(a["content"], a["style"], a["out"], a["B"], a["C"], a["H"], a["W"], a["ws"], a["ws_bytes"], None)

    assert call(content=None) == -1 and call(style=None) == -1 and call(out=None) == -1 and call(ws=None) == -1
    assert call(B=0) == -1 and call(C=0) == -1 and call(H=0) == -1 and call(W=-3) == -1
    assert call(ws_bytes=need - 1) == -1 and call(ws_bytes=0) == -1
    if name.endswith("adain_f32"):
        assert call(H=1, W=1, ws_bytes=1 << 20) == -1                          # unbiased variance needs two pixels


# ---- CLI ------------------------------------------------------------------------------------------------------------------
def test_cli_flag():
    from instantir_amd.infer import apply_color_fix, build_parser
    bp = build_parser()
    a = bp.parse_args(["--test_path", "x"])
    assert a.color_fix == "none" and apply_color_fix(a) == {}
    for m in ("wavelet", "adain"):
        assert apply_color_fix(bp.parse_args(["--test_path", "x", "--color_fix", m])) == {"color_fix": m}
    assert apply_color_fix(bp.parse_args(["--test_path", "x", "--color_fix", "none"])) == {}
    with pytest.raises(SystemExit):
        bp.parse_args(["--test_path", "x", "--color_fix", "histogram"])


def test_demo_handler_takes_color_fix():
    import inspect
    from instantir_amd.demo import instantir_restore
    assert inspect.signature(instantir_restore).parameters["color_fix"].default is None


# ---- pipeline refusals that need no device ----------------------------------------------------------------------------------
def _pipe():
    from instantir_amd.pipeline import InstantIRPipeline
    return InstantIRPipeline(UNetConfig.tiny(), {}, device="cpu")


def _kw():
    return dict(image=torch.zeros(1, 4, 8, 8), prompt_embeds=torch.zeros(1, 77, 64), pooled_prompt_embeds=torch.zeros(1, 32))


def test_color_fix_is_a_named_parameter():
    import inspect
    from instantir_amd.pipeline import InstantIRPipeline
    for fn in (InstantIRPipeline.__call__, InstantIRPipeline.restore_single_step):
        ps = inspect.signature(fn).parameters
        assert ps["color_fix"].default is None and ps["color_fix_reference"].default is None


@pytest.mark.parametrize("mode", ["histogram", "Wavelet", "", 1])
def test_unknown_mode_is_refused_naming_the_three(mode):
    with pytest.raises(ValueError, match="None, 'wavelet' or 'adain'"):
        _pipe()(color_fix=mode, **_kw())


@pytest.mark.parametrize("mode", ["wavelet", "adain"])
def test_latent_output_with_color_fix_is_refused(mode):
    with pytest.raises(ValueError, match="latent"):
        _pipe()(color_fix=mode, output_type="latent", **_kw())


def test_latent_image_needs_a_reference_and_sizes_must_match():
    p = _pipe()
    lat = torch.zeros(1, 4, 8, 8)
    with pytest.raises(ValueError, match="color_fix_reference"):
        p._color_fix_reference(None, lat, 1, 1)
    with pytest.raises(ValueError, match="64, 64"):
        p._color_fix_reference(torch.zeros(1, 3, 32, 32), lat, 1, 1)                 # no resampling
    ref = p._color_fix_reference(torch.rand(1, 3, 64, 64), lat, 4, 2)
    assert ref.shape == (4, 3, 64, 64) and ref.is_contiguous()
    px = torch.rand(2, 3, 16, 16) * 2 - 1
    ref = p._color_fix_reference(None, px, 4, 2)                                       # expanded as lq is: repeat_interleave
    assert torch.equal(ref, (px / 2 + 0.5).clamp(0, 1).repeat_interleave(2, 0))
    one = p._color_fix_reference(None, px[:1], 3, 3)                                   # one image serves the batch
    assert torch.equal(one, (px[:1] / 2 + 0.5).clamp(0, 1).repeat(3, 1, 1, 1))
    with pytest.raises(ValueError, match="batch"):
        p._color_fix_reference(torch.rand(3, 3, 64, 64), lat, 4, 1)
    from PIL import Image
    import numpy as np
    im = Image.fromarray((np.arange(64 * 64 * 3) % 251).astype("uint8").reshape(64, 64, 3))
    ref = p._color_fix_reference(im, lat, 1, 1)
    assert ref.shape == (1, 3, 64, 64) and abs(ref[0, 1, 0, 0].item() - 1 / 255) < 1e-7
