"""CPU: perturbed-attention guidance (PAG) host rules -- layer selection over the SDXL self-attention names, the per-step scale
s_t, argument checks of the new ABI entries (no GPU needed: arguments are rejected before any HIP call), the API switches,
refusals and the CLI flags."""
from types import SimpleNamespace

import pytest

from instantir_amd import pag
from instantir_amd.config import UNetConfig


@pytest.fixture(scope="module")
def sdxl_paths():
    return pag.attn1_paths(UNetConfig.sdxl())


def test_sdxl_attn1_names(sdxl_paths):
    """70 transformer blocks: down 2 x 2 + 2 x 10, mid 10, up 3 x 10 + 3 x 2 (up block 2 has none); diffusers' dotted names."""
    assert len(sdxl_paths) == len(set(sdxl_paths)) == 70
    assert "down_blocks.2.attentions.1.transformer_blocks.3.attn1" in sdxl_paths
    assert "mid_block.attentions.0.transformer_blocks.7.attn1" in sdxl_paths
    assert "up_blocks.1.attentions.2.transformer_blocks.1.attn1" in sdxl_paths
    assert not any(p.startswith("down_blocks.0.") or p.startswith("up_blocks.2.") for p in sdxl_paths)
    assert all(p.endswith(".attn1") for p in sdxl_paths)


@pytest.mark.parametrize("layers,n", [("mid", 10), ("down_blocks.2", 20), ("up_blocks.0", 30), ("up_blocks.1.attentions.2", 2),
                                      (["mid", "up_blocks.0"], 40), (["mid", "mid_block"], 10), ("down_blocks.1", 4),
                                      (r"transformer_blocks\.(0|1)\.attn1", 4 + 4 + 2 + 6 + 6),
                                      ("attn1", 70), ("blocks.1.attentions", 4 + 6)])
def test_layer_counts(sdxl_paths, layers, n):
    assert len(pag.select(layers, sdxl_paths)) == n


def test_selection_keeps_forward_order_and_only_self_attention(sdxl_paths):
    got = pag.select(["up_blocks.0", "mid"], sdxl_paths)
    assert got == [p for p in sdxl_paths if p.startswith("mid_block.") or p.startswith("up_blocks.0.")]
    assert all(".attn1" in p and ".attn2" not in p for p in got)


def test_dot_boundary_rule():
    """A match ends at '.', '_' or the end of the name: down_blocks.1 never selects down_blocks.10..., blocks.1 never
    blocks.10, and a match inside a word selects nothing."""
    names = ["down_blocks.1.attentions.0.transformer_blocks.0.attn1", "down_blocks.10.attentions.0.transformer_blocks.0.attn1",
             "mid_block.attentions.0.transformer_blocks.10.attn1", "mid_block.attentions.0.transformer_blocks.1.attn1"]
    assert pag.select("down_blocks.1", names) == names[:1]
    assert pag.select("down_blocks.10", names) == names[1:2]
    assert pag.select("transformer_blocks.1", names) == names[3:]
    assert pag.select(r"blocks\.1", names) == [names[0], names[3]]
    assert pag.select("transformer_blocks.1.attn1", names) == names[3:]
    assert pag.select("mid", names) == names[2:] and pag.select("down", names) == names[:2]
    for partial in ("down_blocks.1.att", "attn", "mid_bl", "transformer_blocks.1.at"):
        with pytest.raises(ValueError, match="selects no"):
            pag.select(partial, names)


def test_unmatched_entry_and_empty_list_raise(sdxl_paths):
    with pytest.raises(ValueError, match="down_blocks.0"):
        pag.select(["mid", "down_blocks.0"], sdxl_paths)          # the level-0 blocks have no attention
    with pytest.raises(ValueError, match="up_blocks.1.attentions.3"):
        pag.select("up_blocks.1.attentions.3", sdxl_paths)
    with pytest.raises(ValueError, match="empty"):
        pag.select([], sdxl_paths)
    with pytest.raises(ValueError, match="regular expression"):
        pag.select("mid(", sdxl_paths)


@pytest.mark.parametrize("scale,adaptive", [(3.0, 0.0), (3.0, 0.003), (5.0, 0.01), (1.5, 0.1), (0.0, 0.0), (2.0, 0.004)])
def test_scale_table(scale, adaptive):
    """s_t = max(pag_scale - pag_adaptive_scale * (1000 - t), 0) over integer and fractional (Karras) timesteps."""
    ts = [999, 981, 501, 1, 0, 812.37109375, 24.5, 0.73]
    for t in ts:
        want = scale - adaptive * (1000.0 - float(t))
        want = want if want > 0 else 0.0
        got = pag.scale_at(scale, adaptive, t)
        assert got == pytest.approx(want, rel=0, abs=1e-12) and got >= 0.0
    assert pag.scale_at(3.0, 0.0, 0) == 3.0                                     # no adaptive term: constant


# ---- ABI: the new entries reject bad arguments before any HIP call ------------------------------------------------------
def test_ident_attention_rejects_bad_arguments_without_a_gpu():
    import ctypes as C
    from instantir_amd import lib
    h = lib.load()
    P = 4096

    def desc(**kw):
        d = lib.AttnDesc()
        d.Q, d.ldq, d.q_batch_stride = P, 3 * 640, 1024 * 3 * 640
        d.O, d.ldo, d.o_batch_stride = P, 640, 1024 * 640
        d.batch, d.heads, d.Tq, d.nseg, d.scale = 3, 10, 1024, 1, 0.125
        d.kv[0].K, d.kv[0].ldk, d.kv[0].k_batch_stride = P, 3 * 640, 1024 * 3 * 640
        d.kv[0].Vt, d.kv[0].ldvt, d.kv[0].vt_batch_stride, d.kv[0].Tkv = P, 3 * 1024, 1024, 1024
        for k, v in kw.items():
            if k.startswith("kv_"):
                setattr(d.kv[0], k[3:], v)
            else:
                setattr(d, k, v)
        return d

    call = lambda ident, **kw: h.iir_attention_d64_ident_f16(C.byref(desc(**kw)), ident, None)
    for bad in (0, -1, 3, 4):
        assert call(bad) == -1, bad                 # ident_from outside [1, batch)
    assert call(1, batch=1) == -1
    assert call(1, nseg=2) == -1                    # one KV segment only
    assert call(1, causal=1) == -1
    assert call(1, o_fp8=1) == -1
    assert call(1, kv_Tkv=77) == -1                 # identity needs Tkv == Tq
    assert call(1, Q=None) == -1 and call(1, O=None) == -1 and call(1, kv_Vt=None) == -1
    assert call(1, ldq=3 * 640 + 4) == -1 and call(1, ldo=642) == -1 and call(1, kv_ldvt=3 * 1024 + 4) == -1
    assert call(1, kv_vt_batch_stride=1020) == -1
    assert h.iir_attention_d64_ident_f16(None, 1, None) == -1


def test_pag_step_entries_reject_bad_arguments_without_a_gpu():
    import ctypes
    from instantir_amd import lib
    h = lib.load()
    P = 4096
    B, C, HW = 1, 4, 64

    def step(**kw):           # the descriptor spelling of the former iir_sched_step_pag: the PAG bit
        a = dict(eps_nhwc=P, lde=64, B=B, C=C, HW=HW, cfg=1, coef=P, groups=lib.STEP_PAG, pag_scale=P, x=P, prev=P)
        a.update(kw)
        return h.iir_sched_step(ctypes.byref(lib.SchedDesc(**a)), None)

    assert step(pag_scale=None) == -1 and step(eps_nhwc=None) == -1 and step(coef=None) == -1 and step(x=None) == -1
    assert step(B=0) == -1 and step(lde=3) == -1
    assert step(cfg=0, eps_factor=P) == -1          # rescale factor only with CFG
    assert step(groups=0) == -1                     # a pag_scale without its bit
    assert step(groups=lib.STEP_PAG | 16) == -1 and step(groups=lib.STEP_PAG | 1 << 31) == -1      # a bit outside the four
    assert h.iir_sched_step(None, None) == -1

    def hist(**kw):           # ... of iir_sched_step_hist_pag: both bits
        return step(**dict(dict(groups=lib.STEP_PAG | lib.STEP_HIST, hist=P + 1024, prev=P + 2048), **kw))

    assert hist(pag_scale=None) == -1 and hist(hist=None) == -1
    assert hist(hist=P) == -1                       # hist aliases x
    assert hist(prev=P + 1024) == -1                # hist aliases prev
    assert hist(cfg=0, eps_factor=P) == -1 and hist(C=0) == -1
    assert hist(groups=lib.STEP_PAG) == -1          # a hist without its bit

    def r(fac=P, **kw):       # ... of iir_cfg_rescale_factor_pag
        a = dict(eps_nhwc=P, lde=64, B=B, C=C, HW=HW, coef=P, groups=lib.STEP_PAG, pag_scale=P)
        a.update(kw)
        return h.iir_cfg_rescale_factor(ctypes.byref(lib.SchedDesc(**a)), 0.7, fac, None)

    assert r(pag_scale=None) == -1 and r(eps_nhwc=None) == -1 and r(fac=None) == -1 and r(B=0) == -1
    assert h.iir_cfg_rescale_factor(None, 0.7, P, None) == -1
    cs = h.iir_copy_segments
    assert cs(None, 1, 16, None) == -1 and cs(P, 0, 16, None) == -1 and cs(P, 1, 0, None) == -1 and cs(P, 70000, 16, None) == -1


# ---- API switches and refusals --------------------------------------------------------------------------------------------
def _pipe():
    from instantir_amd.pipeline import InstantIRPipeline
    return InstantIRPipeline(UNetConfig.tiny(), {}, device="cpu")


def test_enable_set_disable():
    p = _pipe()
    assert p.pag_applied_layers is None
    p.enable_pag()
    assert p.pag_applied_layers == ["mid"]
    assert p._pag_paths == ("mid_block.attentions.0.transformer_blocks.0.attn1", "mid_block.attentions.0.transformer_blocks.1.attn1")
    p.set_pag_applied_layers(["mid", "up_blocks.0"])
    assert p.pag_applied_layers == ["mid", "up_blocks.0"] and len(p._pag_paths) == 2 + 3 * 2
    with pytest.raises(ValueError, match="up_blocks.2"):          # tiny: up block 2 has no attention
        p.set_pag_applied_layers("up_blocks.2")
    assert p.pag_applied_layers == ["mid", "up_blocks.0"]         # a refused change leaves the setting as it was
    p.disable_pag()
    assert p.pag_applied_layers is None and p._pag_paths is None
    with pytest.raises(ValueError, match="empty"):
        p.enable_pag([])


@pytest.mark.parametrize("kw", [dict(pag_scale=3.0), dict(pag_scale=0.0), dict(pag_adaptive_scale=0.01)])
def test_pag_arguments_without_enable_pag_are_refused(kw):
    import torch
    p = _pipe()
    with pytest.raises(ValueError, match="enable_pag"):
        p(image=torch.zeros(1, 4, 8, 8), prompt_embeds=torch.zeros(1, 77, 64), pooled_prompt_embeds=torch.zeros(1, 32), **kw)


def test_fp8_engines_refuse_pag():
    from instantir_amd.engine import HipUNet
    fp8 = SimpleNamespace(fp8_linear=True, pag=None)
    with pytest.raises(ValueError, match="fp8"):
        pag.check_engine(fp8)
    with pytest.raises(ValueError, match="fp8"):
        HipUNet.set_pag(fp8, {"mid_block.attentions.0.transformer_blocks.0.attn1"}, 2)
    p = _pipe()
    p._unet = fp8
    with pytest.raises(ValueError, match="fp8"):
        p.enable_pag("mid")
    fp16 = SimpleNamespace(fp8_linear=False, pag=None)
    HipUNet.set_pag(fp16, {"a.attn1"}, 2)
    assert fp16.pag == (frozenset({"a.attn1"}), 2)
    HipUNet.set_pag(fp16, None, 0)
    assert fp16.pag is None


def test_cli_pag_flags():
    from instantir_amd.infer import apply_pag, build_parser
    bp = build_parser()
    a = bp.parse_args(["--test_path", "x"])
    assert a.pag_scale == 0.0 and a.pag_adaptive_scale == 0.0 and a.pag_layers == "mid"
    p = _pipe()
    assert apply_pag(p, a) == {} and p.pag_applied_layers is None             # default: off, enable_pag not called
    a = bp.parse_args(["--test_path", "x", "--pag_scale", "2.5", "--pag_adaptive_scale", "0.002", "--pag_layers", "mid, up_blocks.0"])
    p = _pipe()
    assert apply_pag(p, a) == {"pag_scale": 2.5, "pag_adaptive_scale": 0.002}
    assert p.pag_applied_layers == ["mid", "up_blocks.0"]
    p = _pipe()
    apply_pag(p, bp.parse_args(["--test_path", "x", "--pag_scale", "3"]))
    assert p.pag_applied_layers == ["mid"]
    with pytest.raises(SystemExit):
        apply_pag(_pipe(), bp.parse_args(["--test_path", "x", "--pag_adaptive_scale", "0.01"]))
    with pytest.raises(SystemExit):
        apply_pag(_pipe(), bp.parse_args(["--test_path", "x", "--pag_scale", "-1"]))
    with pytest.raises(ValueError, match="down_blocks.0"):
        apply_pag(_pipe(), bp.parse_args(["--test_path", "x", "--pag_scale", "3", "--pag_layers", "down_blocks.0"]))
