"""GPU: every epilogue form of the 8-wave GEMM (csrc/gemm8.hip: GEGLU / plain as separate builds, the GEGLU pair exchange by
v_permlane32_swap, row statistics read from LDS without a test) on its 256 x 320 build (tile 91) and its
256 x 256 build (tile 92), bit for bit against the 4-wave 128 x 160 kernel (tile 24) on the same seeded inputs, and loosely
against torch fp32 (fp16 output rounding 2^-11 plus the fp32 accumulation order: 3e-3 plain, 4e-3 behind a folded LayerNorm,
8e-3 for GEGLU, which multiplies two such quantities -- the bounds of test_gemm8_tile / test_gemm_layernorm_fold).

The weight rows cycle through four scales so that the activation / the GEGLU gate sees every regime of the erf approximation:
ordinary values, |x| up to ~12 and beyond (exp underflow), exact zeros (zero weight row, zero bias) and negative values next to
zero (zero row with a tiny negative bias; rows scaled by 1e-3)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SCALES = (1.0, 4.0, 0.0, 1e-3)
TINY_NEG = -6e-5
ACTS = {"none": lambda y: y, "silu": F.silu, "gelu": F.gelu, "quick": lambda y: y * torch.sigmoid(1.702 * y)}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from instantir_amd import lib
    lib.load()
    return torch.device("cuda:0")


def _close(got, want, tol, what):
    err = (got.float().cpu() - want).abs()
    bad = (err > tol + tol * want.abs()).sum().item()
    assert bad == 0, f"{what}: {bad}/{want.numel()} off, max err {err.max().item():.4g} (ref max {want.abs().max().item():.4g})"


def _operands(seed, M, N, K, geglu, bias=True):
    """a (M, K), w (N, K) in the layout the device reads (GEGLU: 8 value rows, then their 8 gate rows), bias (N) or None, and
    the per-row scale class; the scale classes apply to the gate rows (GEGLU) or to every row (plain)."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(M, K, generator=g).half()
    w = torch.randn(N, K, generator=g) * K ** -0.5
    b = torch.randn(N, generator=g)
    r = torch.arange(N)
    cls = (r // 2) % 4
    if geglu:
        cls = torch.where(r % 16 >= 8, cls, torch.zeros_like(cls))
    w = w * torch.tensor(SCALES)[cls][:, None]
    b = torch.where(cls == 3, torch.zeros_like(b), b)
    b = torch.where(cls == 2, torch.where(r % 2 == 0, torch.zeros_like(b), torch.full_like(b, TINY_NEG)), b)
    return a, w.half(), (b.half() if bias else None), cls


def _check_regimes(x, cls, bias=True):
    """x: the pre-activation values (M, N) of the rows the scale classes apply to"""
    assert x[:, cls == 1].abs().max() >= 11.0
    assert (x[:, cls == 3].abs().max() < 0.05) and (x[:, cls == 3] < 0).any()
    zero_cols = x[:, cls == 2]
    if bias:
        assert (zero_cols == 0).any() and ((zero_cols < 0) & (zero_cols > -1e-4)).any()
    else:
        assert (zero_cols == 0).all()


def _geglu_ref(y):
    yb = y.reshape(y.shape[0], -1, 16)
    return (yb[:, :, :8] * F.gelu(yb[:, :, 8:])).reshape(y.shape[0], -1)


def _folded(dev, seed, M, C, w, b):
    """The raw rows `h` a producing GEMM wrote with its LayerNorm partials, the fold of (gamma, beta) into (w, b), and the
    pre-activation reference LayerNorm(h) . w^T + b from the fold's own fp16 weights."""
    from instantir_amd import ops
    g = torch.Generator().manual_seed(seed)
    a0 = torch.randn(M, C, generator=g).half()
    w0 = (torch.randn(C, C, generator=g) * C ** -0.5).half()
    gamma, beta = (1.0 + 0.2 * torch.randn(C, generator=g)).half(), (0.3 * torch.randn(C, generator=g)).half()
    parts = ops.ln_parts(M, C, C)
    assert 0 < parts <= 8
    stats = torch.zeros(parts, M, 2, dtype=torch.float32, device=dev)
    h = torch.empty(M, C, dtype=torch.half, device=dev)
    ops.gemm(a0.to(dev), w0.to(dev), h, ln_out=stats)
    fold = ops.LnFold(w.to(dev), gamma.to(dev), beta.to(dev), bias=b.to(dev), eps=1e-5)
    torch.cuda.synchronize()
    y = F.layer_norm(h.float().cpu(), (C,), eps=1e-5) @ fold.w.float().cpu().T + fold.bias.float().cpu()
    return h, fold, stats, y


@pytest.mark.parametrize("M,N,K,tile,bias,fold", [(256, 320, 128, 91, True, False), (512, 640, 192, 91, True, True),
                                                  (256, 320, 128, 91, False, False), (512, 512, 128, 92, False, False),
                                                  (256, 512, 192, 92, True, True)])
def test_geglu(dev, M, N, K, tile, bias, fold):
    from instantir_amd import ops
    a, w, b, cls = _operands(M + N + K + tile, M, N, K, True, bias or fold)
    kw = dict(epi=ops.EPI_GEGLU)
    if fold:
        a_dev, f, stats, y = _folded(dev, N + K, M, K, w, b)
        w_dev, kw["bias"], kw["ln_in"] = f.w, f.bias, (stats, f.colsum, f.eps)
    else:
        a_dev, w_dev = a.to(dev), w.to(dev)
        kw["bias"] = b.to(dev) if bias else None
        y = a.float() @ w.float().T + (b.float() if bias else 0.0)
    if not fold:                                         # (behind the fold the bias carries W . beta: no exact zeros there)
        _check_regimes(y, cls, bias)
    out, old = (torch.zeros(M, N // 2, dtype=torch.half, device=dev) for _ in range(2))
    ops.gemm(a_dev, w_dev, out, tile=tile, **kw)
    ops.gemm(a_dev, w_dev, old, tile=24, **kw)
    torch.cuda.synchronize()
    _close(out, _geglu_ref(y), 8e-3, "GEGLU")
    if not fold:                                         # value * gelu(0) is a zero of either sign
        gate_zero = (y == 0).reshape(M, -1, 16)[:, :, 8:].reshape(M, -1)
        assert gate_zero.any() and (out.cpu()[gate_zero] == 0).all()
    assert torch.equal(out, old), "gemm8 differs from the 4-wave kernel"


@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("act", ["none", "silu", "gelu", "quick"])
@pytest.mark.parametrize("N,tile", [(320, 91), (256, 92)])
def test_plain_activations(dev, N, tile, act, res):
    from instantir_amd import ops
    M, K = 256, 128
    a, w, b, cls = _operands(N + tile, M, N, K, False)
    y = a.float() @ w.float().T + b.float()
    _check_regimes(y, cls)
    r = torch.randn(M, N, generator=torch.Generator().manual_seed(N)).half() if res else None
    want = ACTS[act](y) + (r.float() if res else 0.0)
    kw = dict(bias=b.to(dev), act={"none": ops.ACT_NONE, "silu": ops.ACT_SILU, "gelu": ops.ACT_GELU, "quick": ops.ACT_QUICKGELU}[act])
    if res:
        kw["res"] = r.to(dev)
    out, old = (torch.zeros(M, N, dtype=torch.half, device=dev) for _ in range(2))
    ops.gemm(a.to(dev), w.to(dev), out, tile=tile, **kw)
    ops.gemm(a.to(dev), w.to(dev), old, tile=24, **kw)
    torch.cuda.synchronize()
    _close(out, want, 3e-3, f"plain {act}")
    assert torch.equal(out, old), "gemm8 differs from the 4-wave kernel"


def test_plain_layernorm_fold_transposed_v_on_256x256(dev):
    """the fused q|k|v projection as the chooser sends it to the 256 x 256 build: ln_in, the V third written transposed"""
    from instantir_amd import ops
    M, C, N, tr_from = 512, 256, 768, 512
    _, w, b, _ = _operands(7, M, N, C, False)
    h, f, stats, y = _folded(dev, 11, M, C, w, b)
    outs = []
    for tile in (92, 24):
        qk = torch.zeros(M, tr_from, dtype=torch.half, device=dev)
        vt = torch.zeros(N - tr_from, M, dtype=torch.half, device=dev)
        ops.gemm(h, f.w, qk, bias=f.bias, tile=tile, out_t=(vt, tr_from), ln_in=(stats, f.colsum, f.eps))
        outs.append((qk, vt))
    torch.cuda.synchronize()
    _close(outs[0][0], y[:, :tr_from], 4e-3, "q|k")
    _close(outs[0][1], y[:, tr_from:].T, 4e-3, "V^T")
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), "gemm8 differs from the 4-wave kernel"


@pytest.mark.parametrize("M,N,K,mode", [(512, 640, 256, "geglu"), (256, 320, 256, "none"), (512, 640, 256, "silu+res")])
def test_all_fp8_forms(dev, M, N, K, mode):
    """both operands fp8-E4M3 (the 256 x 320 all-fp8 build) against the 4-wave all-fp8 build; reference: the same bytes in fp32"""
    from instantir_amd import ops
    geglu = mode == "geglu"
    a, w, b, cls = _operands(M + N + K, M, N, K, geglu)
    a8, sa = ops.quantize_fp8_tensor(a.to(dev))
    q, sc = ops.quantize_fp8_rows(w.to(dev))
    w8 = ops.Fp8Weight(q, sc)
    y = (a8.float().cpu() * sa) @ (q.float().cpu() * sc.cpu()[:, None]).T + b.float()
    _check_regimes(y, cls)
    r = torch.randn(M, N, generator=torch.Generator().manual_seed(K)).half() if mode == "silu+res" else None
    want = _geglu_ref(y) if geglu else (F.silu(y) + r.float() if r is not None else y)
    kw = dict(a_scale=sa, bias=b.to(dev), epi=ops.EPI_GEGLU if geglu else ops.EPI_PLAIN)
    if r is not None:
        kw.update(res=r.to(dev), act=ops.ACT_SILU)
    out, old = (torch.zeros(M, N // 2 if geglu else N, dtype=torch.half, device=dev) for _ in range(2))
    ops.gemm_fp8(a8, w8, out, tile=91, **kw)
    ops.gemm_fp8(a8, w8, old, tile=24, **kw)
    torch.cuda.synchronize()
    _close(out, want, 8e-3 if geglu else 3e-3, f"all-fp8 {mode}")
    assert torch.equal(out, old), "gemm8 differs from the 4-wave kernel"
