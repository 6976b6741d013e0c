"""GPU: the single-head flash attention of the VAE mid block (`iir_attention_1h`, `HipVAE.enable_flash_attention()`).

Kernel bound on max |O - O64| (O64: fp64 torch on the same 16-bit inputs), the larger of
  derived:  3 u (max|V| + max|bias|), u = 2^-9 (bf16) / 2^-12 (fp16): one rounding of P (a convex combination of V rows, so
            an error of u max|V| at most), one of the output (u (max|V| + max|bias|)), and a 1.5x margin for the fp32 score
            arithmetic (scores up to ~100 at 2^-24 relative, times 512 terms: below 1e-3 in the exponent);
  measured: twice the error of an fp32 restatement with the kernel's rounding points (fp32 scores and softmax, P rounded to the
            element type, fp32 P.V, output rounded) against the same fp64 result on the same inputs.
Both errors of every case are appended to profiles/r09_vae_flash_errors.log.

VAE bars are those of tests/test_vae_gpu.py: pixel PSNR > 47 dB (bf16) / > 65 dB (fp16) against the fp32 oracle."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = {torch.bfloat16: 47.0, torch.float16: 65.0}
U = {torch.bfloat16: 2.0 ** -9, torch.float16: 2.0 ** -12}
NAME = {torch.bfloat16: "bf16", torch.float16: "fp16"}
SIG = 8.0 ** 0.5             # q, k ~ N(0, SIG) per element: scores q.k / sqrt(D) have a standard deviation of SIG^2 = 8
MARGIN = 30.0


def psnr(got, want):
    import inspect
    from conftest import record_psnr
    mse = ((got - want) ** 2).mean().item()
    v = 10 * math.log10(want.abs().max().item() ** 2 / max(mse, 1e-30))
    record_psnr("vae_flash." + inspect.stack()[1].function, v)
    return v


def _log(line):
    try:
        with open(os.path.join(ROOT, "profiles", "r09_vae_flash_errors.log"), "a") as f:
            f.write(line + "\n")
    except OSError:
        pass


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from instantir_amd import lib
    lib.load()
    return torch.device("cuda:0")


# ---- inputs and references -------------------------------------------------------------------------------------------------
def make_inputs(B, Tq, Tkv, D, dt, seed, device="cpu"):
    """q (B,Tq,D), k (B,Tkv,D), v (B,Tkv,D), bias (D) in `dt`.  In every second query row one key is planted whose score beats
    every other key's by >= MARGIN: for rows 0, 4, 8, ... a key of the LAST 8 (the last key tile), for rows 2, 6, ... one of
    the FIRST 8.  The row's q moves along that key's direction until the margin holds after rounding to `dt` (checked in fp64)."""
    g = torch.Generator().manual_seed(seed)
    q = (torch.randn(B, Tq, D, generator=g) * SIG).to(dt).to(device)
    k = (torch.randn(B, Tkv, D, generator=g) * SIG).to(dt).to(device)
    v = torch.randn(B, Tkv, D, generator=g).to(dt).to(device)
    bias = torch.randn(D, generator=g).to(dt).to(device)
    if Tkv >= 2:
        rows = torch.arange(0, Tq, 2, device=device)
        w = min(Tkv, 8)
        tgt = torch.where(rows % 4 == 0, Tkv - 1 - (rows // 4) % w, (rows // 4) % w)
        for b in range(B):
            kd = k[b].double()
            dirn = kd[tgt] / kd[tgt].norm(dim=1, keepdim=True)
            q0 = q[b, rows].double()
            alpha = torch.zeros(rows.numel(), dtype=torch.float64, device=device)
            for _ in range(40):
                qn = (q0 + alpha[:, None] * dirn).to(dt)
                s = qn.double() @ kd.T * D ** -0.5
                sj = s.gather(1, tgt[:, None])[:, 0]
                s.scatter_(1, tgt[:, None], -float("inf"))
                margin = sj - s.max(dim=1).values
                short = margin < MARGIN + 0.5
                if not short.any():
                    break
                alpha[short] += (MARGIN + 2 - margin[short]) / 2.0
            assert (margin >= MARGIN).all(), "planting did not reach the margin"
            q[b, rows] = qn
    return q, k, v, bias


def ref64(q, k, v, bias, chunk=2048):
    """fp64 attention of the 16-bit inputs (in query chunks: nothing of size Tq x Tkv for the large cases)."""
    D = q.shape[-1]
    kd, vd = k.double(), v.double()
    out = []
    for c in range(0, q.shape[1], chunk):
        s = q[:, c:c + chunk].double() @ kd.transpose(1, 2) * D ** -0.5
        out.append(torch.softmax(s, dim=-1) @ vd)
    o = torch.cat(out, dim=1)
    return o if bias is None else o + bias.double()


def restated32(q, k, v, bias, dt, chunk=2048):
    """The kernel's arithmetic restated in fp32 torch: fp32 scores and softmax statistics, P = exp(s - max) rounded to the element
    type for the product, fp32 P.V divided by the fp32 row sum of the unrounded P, bias added, output rounded."""
    D = q.shape[-1]
    kf, vf = k.float(), v.float()
    out = []
    for c in range(0, q.shape[1], chunk):
        s = q[:, c:c + chunk].float() @ kf.transpose(1, 2) * np.float32(D ** -0.5)
        p = torch.exp(s - s.max(dim=-1, keepdim=True).values)
        o = (p.to(dt).float() @ vf) / p.sum(dim=-1, keepdim=True)
        out.append(o)
    o = torch.cat(out, dim=1)
    if bias is not None:
        o = o + bias.float()
    return o.to(dt)


def run_kernel(dev, q, k, v, bias, dt):
    """Q, K, V^T and O as views into larger buffers whose every other element is a NaN bit pattern (O: a sentinel): rows past the
    last token, columns past D, and V^T columns [T, roundup8(T)) of every image.  Returns (O as (B,Tq,D), the whole O buffer)."""
    from instantir_amd import ops
    B, Tq, D = q.shape
    Tkv = k.shape[1]
    Tp = (Tkv + 7) // 8 * 8
    nan = float("nan")
    qb = torch.full((B * Tq + 8, D + 8), nan, dtype=dt, device=dev)
    kb = torch.full((B * Tkv + 8, D + 16), nan, dtype=dt, device=dev)
    vb = torch.full((D + 8, B * Tp + 16), nan, dtype=dt, device=dev)
    ob = torch.full((B * Tq + 8, D + 8), 777.0, dtype=dt, device=dev)
    qb[:B * Tq, :D] = q.reshape(B * Tq, D).to(dev)
    kb[:B * Tkv, :D] = k.reshape(B * Tkv, D).to(dev)
    for b in range(B):
        vb[:D, b * Tp:b * Tp + Tkv] = v[b].T.to(dev)
    ops.attention_1h(qb[:B * Tq, :D], ob[:B * Tq, :D], kb[:B * Tkv, :D], vb[:D, :B * Tp], Tp, B, Tq, Tkv, D ** -0.5,
                     bias=None if bias is None else bias.to(dev))
    torch.cuda.synchronize()
    return ob[:B * Tq, :D].reshape(B, Tq, D), ob


def old_path(dev, q, k, v, bias, dt):
    """The launches the default VAE path runs per image: S = QK^T/sqrt(D) in fp32, row softmax to 16 bits, O = P V + b."""
    from instantir_amd import ops
    B, T, D = q.shape
    out = torch.empty(B, T, D, dtype=dt, device=dev)
    for b in range(B):
        s32 = torch.empty(T, T, dtype=torch.float32, device=dev)
        pr = torch.empty(T, T, dtype=dt, device=dev)
        ops.gemm(q[b].contiguous().to(dev), k[b].contiguous().to(dev), s32, out_scale=D ** -0.5)
        ops.softmax_rows_f32(s32, pr)
        ops.gemm(pr, v[b].T.contiguous().to(dev), out[b], bias=None if bias is None else bias.to(dev))
    torch.cuda.synchronize()
    return out


SHAPES = [(1, 1, 1), (1, 63, 63), (1, 64, 64), (3, 65, 65), (2, 200, 200), (1, 257, 257), (2, 333, 333), (1, 100, 77)]
_cache = {}


def _case(D, dt, shape):
    """Inputs and both references of a case, computed once and shared (with and without bias, reproducibility)."""
    key = (D, dt, shape)
    if key not in _cache:
        B, Tq, Tkv = shape
        q, k, v, bias = make_inputs(B, Tq, Tkv, D, dt, seed=1000 + D + 7 * Tq + Tkv + (dt == torch.float16))
        _cache[key] = (q, k, v, bias, {wb: (ref64(q, k, v, bias if wb else None), restated32(q, k, v, bias if wb else None, dt))
                                       for wb in (False, True)})
    return _cache[key]


def _bound(dt, v, bias, o64, o32):
    derived = 3 * U[dt] * (v.float().abs().max().item() + (0.0 if bias is None else bias.float().abs().max().item()))
    restated = (o32.double() - o64).abs().max().item()
    return max(derived, 2 * restated), derived, restated


@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "b%d_tq%d_tkv%d" % s)
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("D", [128, 512])
def test_kernel_matches_fp64(dev, D, dt, shape, with_bias):
    q, k, v, bias, refs = _case(D, dt, shape)
    bias = bias if with_bias else None
    o64, o32 = refs[with_bias]
    got, ob = run_kernel(dev, q, k, v, bias, dt)
    B, Tq, Tkv = shape
    assert torch.isfinite(got).all(), "non-finite output: a load was not clamped or a masked key contributed"
    assert (ob[B * Tq:] == 777.0).all() and (ob[:, D:] == 777.0).all(), "stored outside the output view"
    err = (got.double().cpu() - o64).abs().max().item()
    bound, derived, restated = _bound(dt, v, bias, o64, o32)
    line = f"D={D} {NAME[dt]} B={B} Tq={Tq} Tkv={Tkv} bias={int(with_bias)} kernel={err:.3e} restated_fp32={restated:.3e} derived={derived:.3e}"
    if Tq == Tkv and Tq % 64 == 0:          # where the default path applies (its P.V GEMM needs a contraction length % 64 == 0)
        old = old_path(dev, q, k, v, bias, dt)
        line += f" old_path={(old.double().cpu() - o64).abs().max().item():.3e}"
    print(line)
    _log(line)
    assert err <= bound, (err, bound)
    if Tkv >= 2:            # a planted row's softmax is one-hot to 1e-13: its output is that key's V row (+ bias), rounded once
        rows = torch.arange(0, Tq, 2)
        w = min(Tkv, 8)
        tgt = torch.where(rows % 4 == 0, Tkv - 1 - (rows // 4) % w, (rows // 4) % w)
        want = v[:, tgt].float() + (0 if bias is None else bias.float())
        assert (got[:, rows].float().cpu() - want).abs().max().item() <= 2 * U[dt] * want.abs().max().item()


@pytest.fixture(scope="module")
def big_case(dev):
    """T = 16400 (512 tiles of 32 keys plus 16; 256 of 64 plus 16), one image, bf16, above the default path's 16384 ceiling.
    References on the device in query chunks: fp32 torch (the assertion's), fp64 and the fp32 restatement (the bound's)."""
    out = {}
    for D in (128, 512):
        q, k, v, bias = make_inputs(1, 16400, 16400, D, torch.bfloat16, seed=77 + D, device=dev)
        f32 = []
        for c in range(0, 16400, 2048):
            s = q[:, c:c + 2048].float() @ k.float().transpose(1, 2) * np.float32(D ** -0.5)
            f32.append(torch.softmax(s, dim=-1) @ v.float())
        o_f32 = torch.cat(f32, dim=1) + bias.float()
        o64 = ref64(q, k, v, bias)
        o32 = restated32(q, k, v, bias, torch.bfloat16)
        out[D] = (q, k, v, bias, o_f32, o64, o32)
    return out


@pytest.mark.parametrize("D", [128, 512])
def test_kernel_above_the_old_ceiling(dev, big_case, D):
    q, k, v, bias, o_f32, o64, o32 = big_case[D]
    dt = torch.bfloat16
    got, _ = run_kernel(dev, q, k, v, bias, dt)
    assert torch.isfinite(got).all()
    err = (got.float() - o_f32).abs().max().item()
    err64 = (got.double() - o64).abs().max().item()
    bound, derived, restated = _bound(dt, v, bias, o64, o32)
    line = f"D={D} bf16 B=1 Tq=16400 Tkv=16400 bias=1 kernel={err64:.3e} kernel_vs_fp32={err:.3e} restated_fp32={restated:.3e} derived={derived:.3e}"
    print(line)
    _log(line)
    assert err <= bound and err64 <= bound, (err, err64, bound)
    again, _ = run_kernel(dev, q, k, v, bias, dt)
    assert torch.equal(got, again), "two launches differ"


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("D", [128, 512])
def test_kernel_is_bit_reproducible(dev, D, dt):
    q, k, v, bias, _ = _case(D, dt, (2, 333, 333))
    a, _ = run_kernel(dev, q, k, v, bias, dt)
    b, _ = run_kernel(dev, q, k, v, bias, dt)
    assert torch.equal(a, b)


def test_ops_wrapper_refuses_bad_operands(dev):
    from instantir_amd import ops
    D, T = 128, 40
    mk = lambda r, c, dt=torch.bfloat16: torch.zeros(r, c, dtype=dt, device=dev)
    q, o, k, vt = mk(T, D), mk(T, D), mk(T, D), mk(D, T)
    with pytest.raises(ValueError):
        ops.attention_1h(q, o, k, mk(D, T, torch.float16), T, 1, T, T, D ** -0.5)                # mixed element types
    with pytest.raises(ValueError):
        ops.attention_1h(q, o, k, vt[:, :36], 40, 1, T, T, D ** -0.5)                            # roundup8(Tkv) columns not inside a row
    with pytest.raises(ValueError):
        ops.attention_1h(q, o, k, vt, T, 1, T, T, D ** -0.5, bias=mk(1, D)[0].float())           # bias of another type
    with pytest.raises(ValueError):
        ops.attention_1h(q, o, mk(T - 1, D), vt, T, 1, T, T, D ** -0.5)                          # k too short
    from instantir_amd.lib import HipLibraryError
    with pytest.raises(HipLibraryError):
        ops.attention_1h(mk(T, 64), mk(T, 64), mk(T, 64), mk(64, T), T, 1, T, T, 0.125)          # no build at D = 64


# ---- the VAE with the switch ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def vae_env(dev, request):
    """Weights are generated IN the build's element type (as tests/test_vae_gpu.py does), so the fp32 oracle sees exactly the
    stored values.  `hv` has the switch on unless a test turns it off (and back on)."""
    return _tiny_vae(dev, request.param)


def _tiny_vae(dev, dt):
    from instantir_amd import weights as W
    from instantir_amd.config import VAEConfig
    from instantir_amd.vae import HipVAE
    vc = VAEConfig.tiny()
    sd = W.synth_state_dict(W.vae_decoder_specs(vc) + W.vae_encoder_specs(vc), 21, dtype=dt)
    hv = HipVAE(vc, sd, dev, dtype=dt)
    assert hv.use_flash_attention is False
    hv.enable_flash_attention()
    return vc, sd, hv


def _P(sd):
    return {k: v.float() for k, v in sd.items()}


def test_vae_decode_and_encode_match_oracle(vae_env):
    from oracle import vae as OV
    vc, sd, hv = vae_env
    g = torch.Generator().manual_seed(3)
    z = torch.randn(2, 4, 8, 8, generator=g)
    want = OV.decode(_P(sd), vc, z)
    got = hv.decode(z).cpu()
    assert got.shape == want.shape == (2, 3, 64, 64)
    p = psnr(got, want)
    assert torch.isfinite(got).all() and p > BAR[hv.dtype], p
    img = torch.rand(2, 3, 64, 64, generator=g) * 2 - 1
    eps = torch.randn(2, 4, 8, 8, generator=g)
    want = OV.encode(_P(sd), vc, img, eps)
    got = hv.encode(img, eps).cpu()
    p = psnr(got, want)
    assert torch.isfinite(got).all() and p > BAR[hv.dtype], p


def test_vae_decode_T_not_a_multiple_of_4(vae_env):
    """(1,4,6,9): T = 54, T % 4 == 2 -- and a batch of two of them (the per-image V^T projection into padded columns)."""
    from oracle import vae as OV
    vc, sd, hv = vae_env
    g = torch.Generator().manual_seed(5)
    z = torch.randn(1, 4, 6, 9, generator=g)
    hv.disable_flash_attention()
    try:
        with pytest.raises(ValueError):
            hv.decode(z)
    finally:
        hv.enable_flash_attention()
    want = OV.decode(_P(sd), vc, z)
    got = hv.decode(z).cpu()
    p = psnr(got, want)
    assert got.shape == (1, 3, 48, 72) and torch.isfinite(got).all() and p > BAR[hv.dtype], p
    z2 = torch.cat([z, torch.randn(1, 4, 6, 9, generator=g)])
    want2 = OV.decode(_P(sd), vc, z2)
    got2 = hv.decode(z2).cpu()
    p2 = psnr(got2, want2)
    assert torch.isfinite(got2).all() and p2 > BAR[hv.dtype], p2
    assert torch.equal(got2[:1], got)                     # no cross-image arithmetic


def test_vae_decode_above_16384_latent_pixels(dev):
    """(1,4,132,128): T = 16896 latent pixels, a 1056 x 1024 image, untiled; bf16 only (the oracle takes seconds at this size)."""
    from oracle import vae as OV
    vc, sd, hv = _tiny_vae(dev, torch.bfloat16)
    g = torch.Generator().manual_seed(6)
    z = torch.randn(1, 4, 132, 128, generator=g)
    hv.disable_flash_attention()
    try:
        with pytest.raises(ValueError):
            hv.decode(z)
    finally:
        hv.enable_flash_attention()
    got = hv.decode(z).cpu()
    want = OV.decode(_P(sd), vc, z)
    p = psnr(got, want)
    assert got.shape == (1, 3, 1056, 1024) and torch.isfinite(got).all() and p > 47.0, p


def test_vae_switch_on_against_off(vae_env):
    vc, sd, hv = vae_env
    g = torch.Generator().manual_seed(7)
    z = torch.randn(2, 4, 16, 16, generator=g)
    on = hv.decode(z).cpu()
    hv.disable_flash_attention()
    try:
        off = hv.decode(z).cpu()
    finally:
        hv.enable_flash_attention()
    p = psnr(on, off)
    assert torch.isfinite(on).all() and p > BAR[hv.dtype], p


def test_vae_tiled_with_switch(vae_env):
    """Tiling keeps deciding by size; the switch changes the attention inside each tile.  Two tiles (16 and 12 latent columns at
    a 128-px tile): the un-blended interior of tile 0 equals decoding that tile alone with the switch on, bit for bit."""
    vc, sd, hv = vae_env
    g = torch.Generator().manual_seed(8)
    z = torch.randn(1, 4, 12, 24, generator=g) * vc.scaling_factor
    hv.tile_sample_size = 128
    hv.enable_tiling()
    try:
        img = hv.decode_latent(z, "pt")
    finally:
        hv.disable_tiling()
        hv.tile_sample_size = 1024
    assert img.shape == (1, 3, 96, 192) and torch.isfinite(img).all()
    zz = z.to(hv.device) / vc.scaling_factor
    alone = (hv.decode(zz[:, :, :, :16].contiguous()) / 2 + 0.5).clamp(0, 1)
    assert torch.equal(img[:, :, :, :96], alone[:, :, :, :96])
    assert hv.use_flash_attention


def test_vae_toggle_off_restores_the_default_bits(vae_env, dev):
    from instantir_amd.vae import HipVAE
    vc, sd, hv = vae_env
    g = torch.Generator().manual_seed(9)
    z = torch.randn(2, 4, 8, 8, generator=g)
    img = torch.rand(1, 3, 64, 64, generator=g) * 2 - 1
    never = HipVAE(vc, sd, dev, dtype=hv.dtype)
    want_d, want_m = never.decode(z).clone(), never.moments(img).clone()
    on = hv.decode(z).clone()
    hv.disable_flash_attention()
    try:
        got_d, got_m = hv.decode(z).clone(), hv.moments(img).clone()
    finally:
        hv.enable_flash_attention()
    assert torch.equal(got_d, want_d) and torch.equal(got_m, want_m)
    assert not torch.equal(on, want_d)                    # (the two attention paths round differently)


def test_vae_refuses_oversized_geometry_before_any_launch(vae_env):
    """The largest activation must stay below 2 GiB (vae.py header): the check runs on the shape alone, before the first
    allocation or launch.  tiny(): widths (64, 64, 128, 128), so the decoder's largest is 64 channels at 64 T pixels."""
    vc, sd, hv = vae_env
    ch = vc.block_out_channels
    n = len(ch)
    per_pixel = max(ch[n - 1 - i] * 4 ** min(i + 1, n - 1) for i in range(n))
    T = -(-(1 << 31) // (2 * per_pixel))                 # the first T that reaches 2 GiB
    side = math.isqrt(T - 1) + 1
    hv._check_flash_geometry("decode", 1, T - 1)
    with pytest.raises(ValueError, match="2 GiB"):
        hv._check_flash_geometry("decode", 1, T)
    with pytest.raises(ValueError, match="2 GiB"):
        hv._check_flash_geometry("encode", 2, T)
    before = torch.cuda.memory_allocated()
    with pytest.raises(ValueError, match="2 GiB"):
        hv.decode(torch.zeros(1, 4, side, side))
    with pytest.raises(ValueError, match="2 GiB"):
        hv.moments(torch.zeros(1, 3, 1, 1).expand(1, 3, 16 * side, 16 * side))
    assert torch.cuda.memory_allocated() == before


def test_pipeline_pixels_in_pixels_out_with_switch(vae_env, dev):
    """tests/test_vae_gpu.py::test_pipeline_pixels_in_pixels_out with `pipe.vae.enable_flash_attention()`: same geometry, same bar.
    The switch survives the call."""
    from instantir_amd import weights as W
    from instantir_amd.config import UNetConfig
    from instantir_amd.pipeline import InstantIRPipeline
    from instantir_amd.schedulers import DDIMScheduler, LCMSingleStepScheduler
    from oracle import pipeline as OP, vae as OV
    vc, vsd, hv = vae_env
    cfg = UNetConfig.tiny()
    sd = W.synth_state_dict(W.unet_specs(cfg), 11)
    sda = W.synth_state_dict(W.aggregator_specs(cfg), 12)
    lora = W.synth_state_dict(W.lora_specs(cfg), 13)
    g = torch.Generator().manual_seed(9)
    B = 1
    img01 = torch.rand(B, 3, 128, 128, generator=g)
    pe = torch.randn(B, cfg.text_len, cfg.cross_attention_dim, generator=g).half().float()
    pooled = torch.randn(B, cfg.pooled_dim, generator=g).half().float()
    feats = torch.randn(2, B, cfg.resampler.seq_len, cfg.resampler.embedding_dim, generator=g).half().float()
    eps = torch.randn(B, 4, 16, 16, generator=g)
    noise = torch.randn(B, 4, 16, 16, generator=g)
    pipe = InstantIRPipeline(cfg, sd, scheduler=DDIMScheduler(), vae=hv, device=dev)
    pipe.aggregator.load_state_dict(sda)
    pipe.prepare_previewers(lora, lora_alpha=8)
    pipe.vae.enable_flash_attention()
    kw = dict(image=img01, prompt_embeds=pe, pooled_prompt_embeds=pooled, ip_adapter_image_embeds=[feats], output_type="pt",
              num_inference_steps=3, guidance_scale=5.0, init_noise=noise, vae_noise=eps,
              previewer_scheduler=LCMSingleStepScheduler.from_config(pipe.scheduler.config))
    got = pipe(**kw).images.float().cpu()
    assert pipe.vae.use_flash_attention
    fixed = pipe(color_fix="wavelet", **kw).images.float().cpu()
    assert pipe.vae.use_flash_attention and fixed.shape == got.shape and torch.isfinite(fixed).all()
    PV = _P(vsd)
    lq = OV.encode(PV, vc, img01 * 2 - 1, eps) * vc.scaling_factor
    L = {k: v.float() for k, v in lora.items()}
    L["scaling"] = 8.0 / cfg.lora_rank
    lat = OP.denoise({k: v.float() for k, v in sd.items()}, {k: v.float() for k, v in sda.items()}, L, cfg, lq, pe, pooled, feats,
                     init_noise=noise, num_inference_steps=3, guidance_scale=5.0, sampler="ddim")
    want = (OV.decode(PV, vc, lat / vc.scaling_factor) / 2 + 0.5).clamp(0, 1)
    assert got.shape == (B, 3, 128, 128)
    p = psnr(got, want)
    assert p > BAR[hv.dtype] - (0 if hv.dtype == torch.bfloat16 else 8), p


def test_cli_flag_equals_python_api(tmp_path, dev):
    from PIL import Image
    import instantir_amd.infer as cli
    src, out = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    Image.fromarray(np.random.default_rng(0).integers(0, 255, (96, 96, 3), dtype=np.uint8)).save(src / "a.png")
    argv = ["--test_path", str(src), "--out_path", str(out), "--synthetic", "tiny", "--num_inference_steps", "4", "--width", "128",
            "--height", "128", "--batch_size", "1", "--cfg", "5.0"]
    args = cli.build_parser().parse_args(argv + ["--vae_flash_attention"])
    orig = cli.resize_img
    cli.resize_img = lambda im, **kw: orig(im, max_side=128, min_side=128, **kw)
    try:
        torch.manual_seed(7)               # the synthetic VAE encode draws its eps from the global generator
        cli.main(args, dev)
        im, size = cli.resize_img(Image.open(src / "a.png").convert("RGB"), width=128, height=128)
    finally:
        cli.resize_img = orig
    got = np.asarray(Image.open(out / "a.png"))

    def twin(flash):
        torch.manual_seed(7)
        pipe, lcm = cli.build_pipeline(args, dev)
        assert pipe.vae.use_flash_attention is False
        if flash:
            pipe.vae.enable_flash_attention()
        cfg = pipe.cfg
        g = torch.Generator().manual_seed(42)
        kw = dict(prompt_embeds=torch.randn(1, cfg.text_len, cfg.cross_attention_dim, generator=g),
                  pooled_prompt_embeds=torch.randn(1, cfg.pooled_dim, generator=g),
                  negative_prompt_embeds=torch.randn(1, cfg.text_len, cfg.cross_attention_dim, generator=g),
                  negative_pooled_prompt_embeds=torch.randn(1, cfg.pooled_dim, generator=g),
                  ip_adapter_image_embeds=[torch.randn(2, 1, cfg.resampler.seq_len, cfg.resampler.embedding_dim, generator=g)])
        rec = pipe(image=[im], num_inference_steps=4, generator=torch.Generator(device=dev).manual_seed(42), guidance_scale=5.0,
                   previewer_scheduler=lcm, preview_start=0.0, control_guidance_end=1.0, **kw).images[0]
        assert pipe.vae.use_flash_attention is flash
        return np.asarray(rec.resize([size[0], size[1]], Image.BILINEAR))

    want = twin(True)
    assert got.shape == want.shape and np.array_equal(got, want)


# ---- SDXL shapes ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sdxl_vae(dev):
    from instantir_amd import weights as W
    from instantir_amd.config import VAEConfig
    from instantir_amd.vae import HipVAE
    vc = VAEConfig.sdxl()
    return vc, HipVAE(vc, W.synth_state_dict(W.vae_decoder_specs(vc), 31, device=dev, dtype=torch.bfloat16), dev)


def test_sdxl_decode_1536x1024_untiled(sdxl_vae):
    """(1,4,192,128): T = 24576 latent pixels at D = 512, untiled; the largest activation is 0.8 GB."""
    vc, hv = sdxl_vae
    g = torch.Generator().manual_seed(10)
    z = torch.randn(1, 4, 192, 128, generator=g)
    hv.enable_flash_attention()
    try:
        a = hv.decode(z).clone()
        b = hv.decode(z)
        assert a.shape == (1, 3, 1536, 1024) and torch.isfinite(a).all()
        assert torch.equal(a, b)
        with pytest.raises(ValueError, match="2 GiB"):
            hv.decode(torch.zeros(1, 4, 256, 256))        # 2048^2: the 2 GiB activation is beyond the verified limit
    finally:
        hv.disable_flash_attention()
    with pytest.raises(ValueError):
        hv.decode(z)


def test_sdxl_1024_switch_on_against_off(sdxl_vae):
    vc, hv = sdxl_vae
    g = torch.Generator().manual_seed(11)
    z = torch.randn(1, 4, 128, 128, generator=g)
    off = hv.decode(z).clone()
    hv.enable_flash_attention()
    try:
        on = hv.decode(z).clone()
    finally:
        hv.disable_flash_attention()
    p = psnr(on, off)
    assert torch.isfinite(on).all() and p > 47.0, p
