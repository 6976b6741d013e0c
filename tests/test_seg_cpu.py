"""CPU: smoothed-energy guidance (SEG) host rules -- kernel length and taps, the fp64 reference against torch's reflect pad +
depthwise conv, the mean-mode cut-off, the API switches and refusals (PAG / SEG exclusivity included), the CLI flags, and the
argument checks of iir_seg_blur_q_f16 (rejected before any HIP call, so no GPU is needed)."""
import math
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

import seg_ref
from instantir_amd import seg
from instantir_amd.config import UNetConfig


@pytest.mark.parametrize("impl", [seg, seg_ref], ids=["host", "ref"])
def test_kernel_length_table(impl):
    for sigma, k in [(0.5, 3), (1.0, 7), (2.5, 15), (10.0, 61)]:
        assert impl.kernel_length(sigma, 1001) == k, sigma
    for n, k in [(32, 33), (8, 9), (7, 7), (2, 3), (1, 1)]:
        assert impl.kernel_length(100.0, n) == k and impl.kernel_length(math.inf, n) == k, n
    for sigma in (0.05, 0.5, 1.0, 3.3, 100.0, 9999.0):
        for n in range(1, 40):
            k = impl.kernel_length(sigma, n)
            assert k % 2 == 1 and k // 2 <= max(n - 1, 0)


@pytest.mark.parametrize("sigma,n", [(0.5, 9), (1.0, 8), (2.5, 12), (10.0, 7), (100.0, 32), (3.0, 2), (1.0, 1), (9999.0, 64)])
def test_weights_sum_to_one_and_are_symmetric(sigma, n):
    w = seg.weights(sigma, n)
    assert len(w) == seg.kernel_length(sigma, n)
    assert abs(math.fsum(w) - 1.0) <= 1e-15 and all(a == b for a, b in zip(w, reversed(w)))
    assert torch.allclose(torch.tensor(w, dtype=torch.float64), seg_ref.weights(sigma, n), rtol=0, atol=1e-15)


def test_reflect_index():
    assert [seg_ref.reflect_index(i, 5) for i in range(-4, 9)] == [4, 3, 2, 1, 0, 1, 2, 3, 4, 3, 2, 1, 0]


@pytest.mark.parametrize("H,W", [(7, 9), (8, 8)])
@pytest.mark.parametrize("sigma", [0.5, 1.0, 2.5, 10.0, 100.0])
def test_reference_equals_reflect_pad_and_depthwise_conv(H, W, sigma):
    g = torch.Generator().manual_seed(H * 100 + W)
    q = torch.randn(2, H, W, 5, generator=g, dtype=torch.float64)
    wy, wx = seg_ref.weights(sigma, H), seg_ref.weights(sigma, W)
    x = q.permute(0, 3, 1, 2)
    x = F.pad(x, (len(wx) // 2, len(wx) // 2, len(wy) // 2, len(wy) // 2), mode="reflect")
    x = F.conv2d(x, wx.view(1, 1, 1, -1).repeat(5, 1, 1, 1), groups=5)
    x = F.conv2d(x, wy.view(1, 1, -1, 1).repeat(5, 1, 1, 1), groups=5)
    assert (seg_ref.blur(q, sigma) - x.permute(0, 2, 3, 1)).abs().max().item() <= 1e-12


def test_mean_mode_cut_off():
    q = torch.randn(2, 4, 6, 3, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    for impl in (seg, seg_ref):
        assert impl.is_mean(1e4) and impl.is_mean(math.inf) and not impl.is_mean(9999.0) and not impl.is_mean(100.0)
    m = seg_ref.seg_q(q, 1e4)
    assert torch.equal(m, seg_ref.seg_q(q, math.inf)) and torch.allclose(m[:, 2, 3], q.mean(dim=(1, 2)), rtol=0, atol=1e-15)
    assert not torch.allclose(seg_ref.seg_q(q, 9999.0), m, rtol=0, atol=1e-9)          # a very wide blur is still not the mean
    assert torch.equal(seg_ref.seg_q(q, 9999.0), seg_ref.blur(q, 9999.0))


def test_level_grids_and_layer_levels():
    cfg = UNetConfig.sdxl()
    assert seg.level_grids(cfg, 128, 128) == [(128, 128), (64, 64), (32, 32)]
    assert seg.level_grids(cfg, 100, 75)[1:] == [(50, 38), (25, 19)]
    lv = {p: seg.path_level(cfg, p) for p in seg.select(["mid", "down_blocks.1", "up_blocks.0", "up_blocks.1"], cfg)}
    assert {v for p, v in lv.items() if p.startswith("mid_block")} == {2}
    assert {v for p, v in lv.items() if p.startswith("down_blocks.1")} == {1}
    assert {v for p, v in lv.items() if p.startswith("up_blocks.0")} == {2}
    assert {v for p, v in lv.items() if p.startswith("up_blocks.1")} == {1}
    seg.check_grids(cfg, seg.select("up_blocks.1", cfg), 256, 256)                       # level 1 of a 2048^2 image: 128 x 128
    with pytest.raises(ValueError, match="128 x 128"):
        seg.check_grids(cfg, seg.select("up_blocks.1", cfg), 264, 256)
    seg.check_grids(cfg, seg.select("mid", cfg), 264, 256)                               # ... its mid block is fine


# ---- API switches and refusals --------------------------------------------------------------------------------------------
def _pipe():
    from instantir_amd.pipeline import InstantIRPipeline
    return InstantIRPipeline(UNetConfig.tiny(), {}, device="cpu")


def _call(p, **kw):
    return p(image=torch.zeros(1, 4, 8, 8), prompt_embeds=torch.zeros(1, 77, 64), pooled_prompt_embeds=torch.zeros(1, 32), **kw)


def test_enable_set_disable():
    p = _pipe()
    assert p.seg_applied_layers is None and p.seg_blur_sigma is None
    p.enable_seg()
    assert p.seg_applied_layers == ["mid"] and p.seg_blur_sigma == 100.0
    assert p._seg_paths == ("mid_block.attentions.0.transformer_blocks.0.attn1", "mid_block.attentions.0.transformer_blocks.1.attn1")
    p.set_seg_applied_layers(["mid", "up_blocks.0"])
    assert p.seg_applied_layers == ["mid", "up_blocks.0"] and len(p._seg_paths) == 2 + 3 * 2 and p.seg_blur_sigma == 100.0
    with pytest.raises(ValueError, match="seg_applied_layers.*up_blocks.2"):       # tiny: up block 2 has no attention
        p.set_seg_applied_layers("up_blocks.2")
    assert p.seg_applied_layers == ["mid", "up_blocks.0"]                         # a refused change leaves the setting as it was
    p.enable_seg("mid", seg_blur_sigma=math.inf)
    assert p.seg_blur_sigma == math.inf
    p.disable_seg()
    assert p.seg_applied_layers is None and p._seg_paths is None and p.seg_blur_sigma is None
    with pytest.raises(ValueError, match="seg_applied_layers is empty"):
        p.enable_seg([])
    assert p.pag_applied_layers is None                                          # PAG's switch is untouched


@pytest.mark.parametrize("sigma", ["3", None, float("nan"), 0.0, -1.0, True])
def test_bad_sigma_is_refused(sigma):
    p = _pipe()
    with pytest.raises(ValueError, match="seg_blur_sigma"):
        p.enable_seg("mid", seg_blur_sigma=sigma)
    assert p.seg_applied_layers is None


@pytest.mark.parametrize("scale", [3.0, 0.0])
def test_seg_scale_without_enable_seg_is_refused(scale):
    with pytest.raises(ValueError, match="enable_seg"):
        _call(_pipe(), seg_scale=scale)


@pytest.mark.parametrize("scale", [-1.0, float("nan"), float("inf"), "x"])
def test_bad_seg_scale_is_refused(scale):
    p = _pipe()
    p.enable_seg()
    with pytest.raises(ValueError, match="seg_scale"):
        _call(p, seg_scale=scale)


def test_pag_and_seg_exclude_each_other():
    p = _pipe()
    p.enable_pag("mid")
    with pytest.raises(ValueError, match="disable_pag"):
        p.enable_seg("mid")
    assert p.seg_applied_layers is None
    p.disable_pag()
    p.enable_seg("mid")
    with pytest.raises(ValueError, match="disable_seg"):
        p.enable_pag("mid")
    assert p.pag_applied_layers is None
    p.disable_seg()
    p.enable_pag("mid")
    assert p.pag_applied_layers == ["mid"]


def test_fp8_engines_refuse_seg():
    from instantir_amd.engine import HipUNet
    fp8 = SimpleNamespace(fp8_linear=True, pag=None, seg=None)
    with pytest.raises(ValueError, match="fp8"):
        seg.check_engine(fp8)
    with pytest.raises(ValueError, match="fp8"):
        HipUNet.set_seg(fp8, {"mid_block.attentions.0.transformer_blocks.0.attn1"}, 2, 100.0, 16, 16)
    p = _pipe()
    p._unet = fp8
    with pytest.raises(ValueError, match="fp8"):
        p.enable_seg("mid")
    fp16 = SimpleNamespace(fp8_linear=False, pag=None, seg=1)
    HipUNet.set_seg(fp16, None, 0)
    assert fp16.seg is None


def test_engine_set_seg_mean_form_and_refusals():
    from instantir_amd.engine import HipUNet
    cfg = UNetConfig.tiny()
    path = "mid_block.attentions.0.transformer_blocks.0.attn1"
    net = SimpleNamespace(fp8_linear=False, pag=None, seg=None, cfg=cfg, device="cpu")
    HipUNet.set_seg(net, [path], 2, math.inf, 16, 16)                           # the mean form packs no taps
    assert net.seg.mean and net.seg.first == 2 and net.seg.paths == frozenset([path]) and net.seg.taps == {}
    with pytest.raises(ValueError, match="first"):
        HipUNet.set_seg(net, [path], 0, 100.0, 16, 16)
    with pytest.raises(ValueError, match="128 x 128"):
        HipUNet.set_seg(net, ["down_blocks.1.attentions.0.transformer_blocks.0.attn1"], 2, 100.0, 258, 16)
    net.pag = (frozenset([path]), 2)
    with pytest.raises(ValueError, match="perturbed"):
        HipUNet.set_seg(net, [path], 2, 100.0, 16, 16)


def test_cli_seg_flags():
    from instantir_amd.infer import apply_pag, apply_seg, build_parser
    bp = build_parser()
    a = bp.parse_args(["--test_path", "x"])
    assert a.seg_scale == 0.0 and a.seg_blur_sigma == 100.0 and a.seg_layers == "mid"
    p = _pipe()
    assert apply_seg(p, a) == {} and p.seg_applied_layers is None                 # default: off, enable_seg not called
    a = bp.parse_args(["--test_path", "x", "--seg_scale", "2.5", "--seg_blur_sigma", "7.5", "--seg_layers", "mid, up_blocks.0"])
    p = _pipe()
    assert apply_seg(p, a) == {"seg_scale": 2.5}
    assert p.seg_applied_layers == ["mid", "up_blocks.0"] and p.seg_blur_sigma == 7.5
    p = _pipe()
    apply_seg(p, bp.parse_args(["--test_path", "x", "--seg_scale", "3", "--seg_blur_sigma", "inf"]))
    assert p.seg_applied_layers == ["mid"] and p.seg_blur_sigma == math.inf
    with pytest.raises(SystemExit):
        apply_seg(_pipe(), bp.parse_args(["--test_path", "x", "--seg_scale", "-1"]))
    with pytest.raises(ValueError, match="seg_applied_layers.*down_blocks.0"):
        apply_seg(_pipe(), bp.parse_args(["--test_path", "x", "--seg_scale", "3", "--seg_layers", "down_blocks.0"]))
    both = bp.parse_args(["--test_path", "x", "--seg_scale", "3", "--pag_scale", "3"])
    p = _pipe()
    apply_pag(p, both)
    with pytest.raises(ValueError, match="disable_pag"):
        apply_seg(p, both)


# ---- ABI ------------------------------------------------------------------------------------------------------------------
def test_blur_entry_rejects_bad_arguments_without_a_gpu():
    from instantir_amd import lib
    h = lib.load()
    P = 4096
    base = dict(q=P, ldq=2560, images=2, H=32, W=32, C=1280, wy=P, ky=33, wx=P, kx=33, mean=0)

    def call(**kw):
        a = dict(base, **kw)
        return h.iir_seg_blur_q_f16(a["q"], a["ldq"], a["images"], a["H"], a["W"], a["C"], a["wy"], a["ky"], a["wx"], a["kx"],
                                    a["mean"], None)
    assert call(q=None) == -1 and call(wy=None) == -1 and call(wx=None) == -1
    assert call(q=P + 8) == -1                                                     # 16-byte alignment of the first row
    assert call(images=0) == -1 and call(H=0) == -1 and call(W=-1) == -1 and call(C=0) == -1
    assert call(C=1284) == -1                                                      # C % 8
    assert call(ldq=1272) == -1 and call(ldq=2564) == -1                           # ldq < C, ldq % 8
    assert call(ky=32) == -1 and call(kx=0) == -1 and call(kx=4) == -1             # even / empty kernels
    assert call(ky=65) == -1 and call(H=16, ky=33) == -1 and call(W=1, kx=3) == -1  # k // 2 > n - 1
    assert call(H=129, ky=1) == -1 and call(W=256, kx=1) == -1                     # beyond IIR_SEG_MAX_EXTENT
    assert call(mean=1, H=129) == -1 and call(mean=1, q=None) == -1 and call(mean=1, C=12) == -1


def test_abi_version_is_still_3():
    from instantir_amd import lib
    assert lib.load().iir_abi_version() == 3 and "iir_seg_blur_q_f16" in lib.declared_symbols()
