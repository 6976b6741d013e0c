"""fp64 restatement of one `ops.gemm` / `ops.gemm_fp8` / `ops.conv2d` launch, with a per-element error bound derived from the
number formats.  Plain helper for tests/test_gemm_conv_ref_cpu.py and tests/test_gemm_conv_every_build_gpu.py; no GPU use.

`reference(kind, spec)`: `kind` is "gemm", "gemm_fp8" or "conv", `spec` the keyword arguments of that wrapper as CPU tensors
(without `out`, `tile`, `prefetch`; `out_t` is the integer `tr_from`; `w8` is `(q, scale)`; `out_dtype=torch.float32` asks for
the fp32 output form).  It returns a `Ref` whose fields are float64 in the LOGICAL layout (M, N) -- (M, N / 2) for the paired
epilogues -- with `rows[m]` the physical output row of logical row m (`y_img_rows`):

  p      the value before the first rounding, from the 2-byte (or fp8) operands as stored:
           GEMM  a @ w.T;  conv: the NHWC implicit GEMM of the header comment of csrc/gemm_conv.hip, written out directly --
           row m = output pixel (img, oy, ox), k = (ky * ks + kx) * Cin + c, zero padding, `stride`, `ups` (coordinates in the
           2x domain, source pixel (iy >> 1, ix >> 1)), pad_mode = 1 (pad right / bottom only), read from the input's storage by
           its own pixel stride and image stride;
           * wscale[n] * a_scale (fp8 forms; the fp8-weight form first rounds the activations to E4M3 as the kernel does);
           bias, row bias [m // rows_per_rb]; the activation (SiLU, exact-erf GELU, x * sigmoid(1.702 x));
           paired epilogues on the `pair_rows` layout: GEGLU value * gelu(gate), SFT h * (gamma + 1) + beta.
           With `ln_in = (partials, colsum, eps)` (GEMM only) the value before the activation is the LayerNorm fold
           rstd * (a @ w.T - mean * colsum) + bias; it and its shift are restated in tests/gemm_fused_ref.py (`ln_fold`), which also
           holds the references of the statistics a launch leaves (`ln_out`, `gn_out`).
  want   what the kernel stores under its documented order (epilogue comment of gemm_conv.hip): y1 = round_E(p), then
           round_E((y1 + res) * out_scale), `res` read through the `res_img_rows` remap; paired epilogues round once (then times
           out_scale); fp32 output: p * out_scale unrounded.  Columns >= tr_from of an `out_t` launch are the caller's to transpose.
  bound  the per-element bound on |got - want| (below);  first_order: the closed form it replaces (kept for comparison).
  lo, hi the admitted interval of stored values itself (2-byte outputs; bound = max(hi - want, want - lo) + tiny): what a consumer
           of the stored tile may have been handed (tests/xattn_ref.py: the q of the cross-attention epilogue).

The bound.  Let u = 2^-11 (fp16) / 2^-8 (bf16) be the unit roundoff of the element type E, S = sum_k |a_mk * w_nk| (times the
scales), g = K * 2^-24 the fp32 accumulation bound, L the activation's Lipschitz constant (1.13 for SiLU / GELU / quick-GELU, 1
otherwise) and
    d = 2 * g * S * L  (+ C_GELU * |value| where erf-GELU is evaluated)
the largest shift the kernel's fp32 value p' may have against p: g * S * L is the worst case of ANY summation order of the K
products pushed through the activation; the factor 2 leaves the same again for the fp32 epilogue arithmetic (scale, bias and
row-bias adds, v_exp / v_rcp of the activations, each a few 2^-24 relative).  For GEGLU the product rule gives
d = 2 * (|gelu(gate)| * g S_value + |value| * 1.13 * g S_gate + the product of the two), for SFT 2 * (|h| * g S_gamma + g S_beta).

First-order form: |got - want| <= u |p| + u |want| + d + tiny (one term per rounding, one for the shift; tiny = one subnormal
step of E).  It is NOT a bound: when p' and p lie on different sides of a rounding tie, y1 moves by a whole ulp(p), which is up
to 2 u |p|, and the second rounding can add a whole ulp(want).  Where the residual cancels (|want| << |p|) and p sits low in its
binade that exceeds the form; the fp32 stand-in of tests/test_gemm_conv_ref_cpu.py -- a correct kernel by construction -- breaks
it (13 of 327680 elements at the K = 64 shape of the 2 GiB test, 1 to 11 at nine other residual shapes), and doubling the two u terms
would hide a residual added before the first rounding.  So the bound is the exact image of the shift interval under the two
(monotone) roundings:
    y1' in [round_E(p - d), round_E(p + d)]  =>  got in [round_E((round_E(p - d) + res) * s), round_E((round_E(p + d) + res) * s)]
    bound = max(hi - want, want - lo) + tiny
No absolute term, no factor on u: the admitted values are exactly the E values whose rounding cells meet [p - d, p + d].  This is
not bit-exactness.  At K = 320, d is about 5e-4: half an fp16 ulp at 1.0 and tens of ulps near 0.01, so for fp16 almost every
element has a tie inside d and the bound is one to several ulps there (the issue's own shift term); only where ulp(p) >> d -- bf16
throughout, fp16 at K = 64 -- do most elements have to be stored exactly.  (fp32 output: bound = s * d + 2 * 2^-24 * |want|.)  out_scale must be positive.

C_GELU.  `gelu_erf_f` (csrc/common.h) evaluates erf by Abramowitz-Stegun 7.1.26; its error cannot be derived here, so launches
that evaluate it add C_GELU * |value| to d (value: the GEGLU value operand; the pre-activation for ACT_GELU).  Measured on one
MI355X, from the kernels' outputs, on the tile-0 GELU cases of the GPU file (GEGLU (d) at both shapes and ACT_GELU on GEMM (a) / conv (a), fp16, bf16, fp8
forms; 14 launches) with C_GELU = 0: no element of any of them lay outside the bound, so the largest excess
(|got - want| - bound) / |value| is not positive: MEASURED_C_GELU = 0 and C_GELU = 2 x that = 0.  The approximation's error (a few
1e-7 |x|) disappears in the factor 2 of d.  (The project allows GEGLU 8e-3 in test_gemm8_tile; C_GELU must stay below it.)

Room left, one MI355X, the outputs of the kernels (not of the stand-in) over all cases of tests/test_gemm_conv_every_build_gpu.py
(74 tests, 3.7 s wall), per element type, as that file prints them:
              elements     != want         largest |got - want| / bound     largest |got - want| / first-order form
  fp16        36 445 520   4.2 %           0.99998                          1.38
  bf16        14 735 520   4.1 %           1.0                              1.51
  fp8 weights  6 994 400   3.2 %           0.99999                          1.42
  all-fp8      8 456 320   3.4 %           0.99999                          1.20
About 96 % of the stored values are `want` itself; the others lie inside the bound, the worst of them a whole admitted step away
(a step against step + tiny: hence the ratios just under 1, which by construction cannot say more).  The last column shows the
kernels, like the stand-in, outside the first-order form.
"""
import collections

import numpy as np
import torch

EPI_PLAIN, EPI_GEGLU, EPI_SFT = 0, 1, 2
ACT_NONE, ACT_SILU, ACT_GELU, ACT_QUICKGELU = 0, 1, 2, 3
FP8_MAX = 448.0

MEASURED_C_GELU = 0.0          # largest excess over the bound on the tile-0 GELU cases: none (see the docstring)
C_GELU = 2 * MEASURED_C_GELU

LIPSCHITZ = {ACT_NONE: 1.0, ACT_SILU: 1.13, ACT_GELU: 1.13, ACT_QUICKGELU: 1.13}
UNIT = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
TINY = {torch.float16: 2.0 ** -24, torch.bfloat16: 2.0 ** -133}

Ref = collections.namedtuple("Ref", "p want bound first_order rows dtype lo hi", defaults=(None, None))


def round_e(x, dtype):
    """float64 -> the nearest value of `dtype` (ties to even), back in float64.  fp16 straight from fp64 (numpy); bf16 through fp32
    (the fp32 step can move a value only if it lies within 2^-24 relative of a bf16 tie: inside every interval taken here)."""
    if dtype == torch.float16:
        return torch.from_numpy(x.numpy().astype(np.float16).astype(np.float64))
    return x.float().to(torch.bfloat16).double()


def to_e4m3(x):
    """E4M3 (OCP) rounding of fp16 activations, round to nearest even, saturating: what the fp8-weight build applies per fragment."""
    return x.float().clamp(-FP8_MAX, FP8_MAX).to(torch.float8_e4m3fn).float().double()


def gelu(x):
    return 0.5 * x * (1.0 + torch.special.erf(x * 0.7071067811865476))


def activation(x, act):
    if act == ACT_SILU:
        return x * torch.sigmoid(x)
    if act == ACT_GELU:
        return gelu(x)
    if act == ACT_QUICKGELU:
        return x * torch.sigmoid(1.702 * x)
    return x


def conv_out_size(H, W, ksize=3, stride=1, upsample=False, pad_mode=0):
    pad = 0 if pad_mode == 1 else ksize // 2
    pad_hi = 1 if pad_mode == 1 else pad
    Hi, Wi = (2 * H, 2 * W) if upsample else (H, W)
    return (Hi + pad + pad_hi - ksize) // stride + 1, (Wi + pad + pad_hi - ksize) // stride + 1


def im2col(x, ksize=3, stride=1, upsample=False, pad_mode=0):
    """The A matrix of the implicit GEMM, (R * Ho * Wo, ks * ks * Cin) float64, gathered from x's STORAGE by its strides."""
    R, H, W, Cin = x.shape
    ldx, img_stride = x.stride(2), x.stride(0)
    assert x.stride(3) == 1 and x.stride(1) == W * ldx, "NHWC view with dense rows"
    flat = torch.empty(0, dtype=x.dtype).set_(x.untyped_storage()).double()
    pad = 0 if pad_mode == 1 else ksize // 2
    Hi, Wi = (2 * H, 2 * W) if upsample else (H, W)
    Ho, Wo = conv_out_size(H, W, ksize, stride, upsample, pad_mode)
    m = torch.arange(R * Ho * Wo)
    img, rem = m // (Ho * Wo), m % (Ho * Wo)
    oy, ox = rem // Wo, rem % Wo
    c = torch.arange(Cin)
    A = torch.zeros(R * Ho * Wo, ksize * ksize * Cin, dtype=torch.float64)
    for tap in range(ksize * ksize):
        ky, kx = tap // ksize, tap % ksize
        iy, ix = oy * stride - pad + ky, ox * stride - pad + kx
        ok = (iy >= 0) & (iy < Hi) & (ix >= 0) & (ix < Wi)
        pix = (iy >> 1) * W + (ix >> 1) if upsample else iy * W + ix
        idx = x.storage_offset() + img * img_stride + pix * ldx
        idx = torch.where(ok, idx, torch.zeros_like(idx))
        A[:, tap * Cin:(tap + 1) * Cin] = torch.where(ok[:, None], flat[idx[:, None] + c[None, :]], torch.zeros((), dtype=torch.float64))
    return A


def image_rows(M, hw, img_rows):
    """Physical row of logical row m when image i's rows start at i * img_rows (0: dense)."""
    m = torch.arange(M)
    return m if not img_rows else (m // hw) * img_rows + m % hw


def unpair(v):
    """Columns of the `pair_rows` layout -> (value columns, partner columns), each (M, N / 2) in output order."""
    M, N = v.shape
    q = v.reshape(M, N // 16, 2, 8)
    return q[:, :, 0, :].reshape(M, N // 2), q[:, :, 1, :].reshape(M, N // 2)


def reference(kind, spec, c_gelu=None):
    c_gelu = C_GELU if c_gelu is None else c_gelu
    s = dict(spec)
    epi, act = s.get("epi", EPI_PLAIN), s.get("act", ACT_NONE)
    out_scale = float(s.get("out_scale", 1.0))
    assert out_scale > 0, "the interval bound takes a positive out_scale"
    res, hw, res_img_rows, y_img_rows = s.get("res"), 1, 0, 0
    scale = None
    if kind == "conv":
        x, w = s["x"], s["w"]
        dt = x.dtype
        geo = dict(ksize=s.get("ksize", 3), stride=s.get("stride", 1), upsample=bool(s.get("upsample", False)), pad_mode=s.get("pad_mode", 0))
        A = im2col(x, **geo)
        Wm = w.double().reshape(w.shape[0], -1)
        Ho, Wo = conv_out_size(x.shape[1], x.shape[2], **geo)
        hw, res_img_rows, y_img_rows = Ho * Wo, s.get("res_img_rows", 0), s.get("y_img_rows", 0)
    elif kind == "gemm":
        a, w = s["a"], s["w"]
        dt = a.dtype
        if s.get("wscale") is not None:          # fp8 weights, fp16 activations rounded to E4M3 in registers
            A, Wm, scale = to_e4m3(a), w.float().double(), s["wscale"].double()
        else:
            A, Wm = a.double(), w.double()
    elif kind == "gemm_fp8":
        q, wscale = s["w8"]
        dt = torch.float16
        A, Wm, scale = s["a8"].float().double(), q.float().double(), wscale.double() * float(s.get("a_scale", 1.0))
    else:
        raise ValueError(kind)
    M, K = A.shape
    N = Wm.shape[0]
    g = K * 2.0 ** -24
    v = A @ Wm.T
    S = A.abs() @ Wm.abs().T
    if scale is not None:
        v, S = v * scale[None, :], S * scale.abs()[None, :]
    fold = None
    if s.get("ln_in") is not None:          # the LayerNorm fold: restated, with its shift, in tests/gemm_fused_ref.py
        import gemm_fused_ref
        assert kind == "gemm" and s.get("rowbias") is None and s.get("out_dtype") is None and epi != EPI_SFT, "ln_in: a GEMM without row bias, 2-byte output"
        v, fold = gemm_fused_ref.ln_fold(s, v, S, g)          # v: rstd * (a w^T - mean colsum) + bias; fold: its shift
    elif s.get("bias") is not None:
        v = v + s["bias"].double()[None, :]
    if s.get("rowbias") is not None:
        v = v + s["rowbias"].double()[torch.arange(M) // s.get("rows_per_rb", 1)]
    res_rows = image_rows(M, hw, res_img_rows)
    rows = image_rows(M, hw, y_img_rows)
    u, tiny = UNIT[dt], TINY[dt]

    if epi == EPI_PLAIN:
        p = activation(v, act)
        d = 2 * g * S * LIPSCHITZ[act] if fold is None else fold * LIPSCHITZ[act]
        if act == ACT_GELU:
            d = d + c_gelu * v.abs()
        r = res.double()[res_rows] if res is not None else torch.zeros((), dtype=torch.float64)
        if s.get("out_dtype") == torch.float32:
            want = p * out_scale
            bound = out_scale * d + 2 * 2.0 ** -24 * want.abs() + 2.0 ** -149
            return Ref(p, want, bound, bound, rows, torch.float32)
        second = lambda y1: round_e((y1 + r) * out_scale, dt)
    else:
        val, par = unpair(v)
        Sv, Sp = unpair(S)
        if epi == EPI_GEGLU and fold is not None:          # the product rule on the two folded shifts
            p = val * gelu(par)
            dv, dp = unpair(fold)
            d = gelu(par).abs() * dv + val.abs() * 1.13 * dp + 1.13 * dv * dp + c_gelu * val.abs()
        elif epi == EPI_GEGLU:
            p = val * gelu(par)
            d = 2 * (gelu(par).abs() * g * Sv + val.abs() * 1.13 * g * Sp + 1.13 * g * Sv * g * Sp) + c_gelu * val.abs()
        elif epi == EPI_SFT:
            h = res.double()[res_rows]
            p = h * (val + 1.0) + par
            d = 2 * (h.abs() * g * Sv + g * Sp)
        else:
            raise ValueError(epi)
        second = lambda y1: round_e(y1 * out_scale, dt)          # one rounding; phase 2 only scales
    want = second(round_e(p, dt))
    lo, hi = second(round_e(p - d, dt)), second(round_e(p + d, dt))
    bound = torch.maximum(hi - want, want - lo) + tiny
    first_order = u * p.abs() + u * want.abs() + d + tiny
    return Ref(p, want, bound, first_order, rows, dt, lo, hi)


def compare(got, want, bound):
    """(number of elements with |got - want| > bound or a non-finite `got`, the worst of them as a dict or None)."""
    got, want, bound = got.double(), want.double(), bound.double()
    err = (got - want).abs()
    err = torch.where(torch.isfinite(got), err, torch.full_like(err, float("inf")))
    bad = err > bound
    n = int(bad.sum())
    if n == 0:
        return 0, None
    excess = torch.where(bad, err / bound, torch.zeros_like(err))
    i = int(excess.argmax())
    idx = tuple(int(k) for k in np.unravel_index(i, tuple(got.shape)))
    return n, dict(index=idx, got=float(got.reshape(-1)[i]), want=float(want.reshape(-1)[i]), bound=float(bound.reshape(-1)[i]))


def room(got, want, bound):
    """Largest |got - want| / bound."""
    return float(((got.double() - want).abs() / bound).max())


# ---- the seeded launches of tests/test_gemm_conv_every_build_gpu.py (and of the stand-in / mutant tests on the CPU) ----------------
# Standard normals, weights scaled by K^-0.5; A-side operands are views of wider buffers (lda > K, pixel stride > Cin); `res`
# carries minus the column's bias plus half-width noise, so that part of the outputs cancel to near zero: the elements an
# absolute tolerance cannot see.
DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16}
G1, G2, G8, GK = (300, 336), (512, 640), (256, 1280), 320          # K = 5 K tiles: a 4-deep ring refills (all-fp8: 640 bytes)
BIG = (512, 640, 64)                                               # the 2 GiB store switch (K = 128 on the 8-wave kernel: its minimum)
Case = collections.namedtuple("Case", "kind spec")


def _gen(name):
    return torch.Generator().manual_seed(int.from_bytes(name.encode(), "little") % (2 ** 31 - 1))


def _rand(g, *shape, scale=1.0, dtype=torch.float16):
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def wide(t, extra=8):
    """The same values as a view of a buffer with a longer innermost row."""
    big = torch.zeros(*t.shape[:-1], t.shape[-1] + extra, dtype=t.dtype)
    big[..., :t.shape[-1]] = t
    return big[..., :t.shape[-1]]


def quantize_fp8_rows(w):
    scale = (w.float().abs().amax(dim=1).clamp_min(1e-12) / FP8_MAX).contiguous()
    return (w.float() / scale[:, None]).clamp(-FP8_MAX, FP8_MAX).to(torch.float8_e4m3fn).contiguous(), scale


def quantize_fp8_tensor(x):
    scale = float(x.float().abs().amax().clamp_min(1e-12) / FP8_MAX)
    return (x.float() / scale).clamp(-FP8_MAX, FP8_MAX).to(torch.float8_e4m3fn).contiguous(), scale


def _res(g, M, N, bias, dtype, paired=False):
    off = 0.0 if bias is None or paired else -bias.float()[None, :N]
    return (0.5 * torch.randn(M, N, generator=g) + off).to(dtype)


def gemm_case(form, what, M, N, K=GK):
    """form: f16 / bf16 / w8 (fp8 weights) / f8 (all-fp8).  what: full (bias + row bias + residual + SiLU, out_scale 0.5; the all-fp8
    wrapper has neither row bias nor out_scale), res (bias + residual), geglu, out_t (tr_from = 2 N / 3), f32, gelu, quickgelu."""
    g = _gen(f"gemm.{form}.{what}.{M}x{N}x{K}")
    dt = DTYPES.get(form, torch.float16)
    bias = None if what == "f32" else _rand(g, N, dtype=dt)
    if form == "f8":
        a8, sa = quantize_fp8_tensor(_rand(g, M, 2 * K))
        spec = dict(a8=wide(a8.view(torch.uint8), 16).view(torch.float8_e4m3fn), a_scale=sa, w8=quantize_fp8_rows(_rand(g, N, 2 * K, scale=(2 * K) ** -0.5)))
        kind = "gemm_fp8"
    else:
        spec = dict(a=wide(_rand(g, M, K, dtype=dt)))
        w = _rand(g, N, K, scale=K ** -0.5, dtype=dt)
        if form == "w8":
            spec["w"], spec["wscale"] = quantize_fp8_rows(w)
        else:
            spec["w"] = w
        kind = "gemm"
    if bias is not None:
        spec["bias"] = bias
    if what in ("full", "gelu", "quickgelu"):
        spec.update(res=_res(g, M, N, bias, dt), act={"full": ACT_SILU, "gelu": ACT_GELU, "quickgelu": ACT_QUICKGELU}[what])
        if kind == "gemm":
            spec.update(rowbias=_rand(g, (M + 3) // 4, N, dtype=dt), rows_per_rb=4, out_scale=0.5)
    elif what == "res":
        spec.update(res=_res(g, M, N, bias, dt))
    elif what == "geglu":
        spec.update(epi=EPI_GEGLU)
    elif what == "out_t":
        spec.update(out_t=2 * N // 3)
    elif what == "f32":
        spec.update(out_scale=0.5, out_dtype=torch.float32)
    else:
        raise ValueError(what)
    return Case(kind, spec)


def conv_case(form, what, R=2, H=10, W=14, Cin=64, Cout=168):
    """what: full (3x3, bias + per-image row bias + residual + SiLU), res (bias + residual), stride2, stride2_pad1, upsample, 1x1,
    remap (full with y_img_rows = HW + 64, res_img_rows = HW + 128 and a padded image stride), sft, gelu, quickgelu."""
    g = _gen(f"conv.{form}.{what}.{R}x{H}x{W}x{Cin}x{Cout}")
    dt = DTYPES[form]
    ks = 1 if what == "1x1" else 3
    geo = dict(ksize=ks, stride=2 if what.startswith("stride2") else 1, upsample=what == "upsample", pad_mode=1 if what == "stride2_pad1" else 0)
    Ho, Wo = conv_out_size(H, W, **geo)
    hw, M = Ho * Wo, R * Ho * Wo
    x = _rand(g, R, H, W, Cin, dtype=dt)
    if what == "remap":          # pixel stride Cin + 64 and three spare pixels between images
        ldx = Cin + 64
        flat = torch.zeros(R * (H * W + 3) * ldx, dtype=dt)
        xv = torch.as_strided(flat, (R, H, W, Cin), ((H * W + 3) * ldx, W * ldx, ldx, 1))
        xv.copy_(x)
    else:
        xv = wide(x, 64)
    bias = _rand(g, Cout, dtype=dt)
    spec = dict(x=xv, w=_rand(g, Cout, ks, ks, Cin, scale=(ks * ks * Cin) ** -0.5, dtype=dt), bias=bias, **geo)
    if what in ("full", "remap", "gelu", "quickgelu"):
        spec.update(rowbias=_rand(g, R, Cout, dtype=dt), rows_per_rb=hw, act={"gelu": ACT_GELU, "quickgelu": ACT_QUICKGELU}.get(what, ACT_SILU))
    if what == "sft":
        spec.update(epi=EPI_SFT, res=_rand(g, M, Cout // 2, dtype=dt))
    elif what == "remap":
        spec.update(y_img_rows=hw + 64, res_img_rows=hw + 128)
        res = torch.zeros(R * (hw + 128), Cout, dtype=dt)
        res[image_rows(M, hw, hw + 128)] = _res(g, M, Cout, bias, dt)
        spec.update(res=res)
    else:
        spec.update(res=_res(g, M, Cout, bias, dt))
    return Case("conv", spec)


def gemm_cases(form):
    """name -> Case: what every build of `form` runs (the GPU file adds the non-vector write-out of `b` as a layout of its own)."""
    out = {"a": gemm_case(form, "full", *G1), "b": gemm_case(form, "res", *G2),
           "d1": gemm_case(form, "geglu", *G1), "d2": gemm_case(form, "geglu", *G2)}
    if form in DTYPES:
        out.update(e1=gemm_case(form, "out_t", 512, 480), e2=gemm_case(form, "out_t", 512, 960), f=gemm_case(form, "f32", *G1))
    return out


def gemm8_cases(form):
    return {"g8_res": gemm_case(form, "res", *G8), "g8_geglu": gemm_case(form, "geglu", *G8)}


def conv_cases(form):
    """(c1: pad_mode = 1 on the odd 11 x 15 map, whose last taps end ON the last row and column; c2: the same on 10 x 14, where
    they read the padding.)"""
    return {"a": conv_case(form, "full"), "b": conv_case(form, "res", H=16, W=16, Cout=640),
            "c0": conv_case(form, "stride2"), "c1": conv_case(form, "stride2_pad1", H=11, W=15), "c2": conv_case(form, "stride2_pad1"), "d": conv_case(form, "upsample", H=5, W=7),
            "e1": conv_case(form, "1x1"), "e2": conv_case(form, "1x1", Cin=128), "f": conv_case(form, "remap")}


def sft_case():
    return conv_case("f16", "sft", Cout=176)


def act_cases(form):
    return {"gemm.gelu": gemm_case(form, "gelu", *G1), "gemm.quickgelu": gemm_case(form, "quickgelu", *G1),
            "conv.gelu": conv_case(form, "gelu"), "conv.quickgelu": conv_case(form, "quickgelu")} if form in DTYPES else \
           {"gemm.gelu": gemm_case(form, "gelu", *G1), "gemm.quickgelu": gemm_case(form, "quickgelu", *G1)}


def big_case(K=BIG[2]):
    return gemm_case("f16", "res", BIG[0], BIG[1], K)
