"""fp64 restatement of the exported entries of csrc/pointwise.hip (all but `iir_sched_step`, `iir_apg_project*` and the timing
entries), with a per-element bound derived from the number formats and the kernels' own operation counts, numpy / torch fp32
stand-ins of the kernels with one-fault mutants, and the case table of tests/test_pointwise_every_entry_gpu.py.  Plain helper for
that file and for tests/test_pointwise_ref_cpu.py; no GPU use.

The formulas are the reference's, not the kernels':
  sinusoid     module/min_sdxl.py:205-224 (Timesteps): [cos | sin] of t * exp(-ln(1e4) k / half), with the exact ln 1e4 (the kernel
               has an fp32 constant)
  silu         nn.SiLU: x / (1 + exp(-x))
  blend        module/diffusers_vae/autoencoder_kl.py:311-321 (blend_v / blend_h)
  lcm_step     schedulers/lcm_single_step_scheduler.py:455-484, epsilon prediction, no clipping; row r of the CFG-repeated batch
               belongs to image r % B (pipelines/sdxl_instantir.py: cat([latents] * 2))
  rescale      pipelines/sdxl_instantir.py:181-192 (rescale_noise_cfg): phi * std(text) / std(cfg) + (1 - phi), torch.std (N - 1)
  copy_add, pack, unpack, transpose, copy_segments, axpby, sched_step_f32: data movement and linear forms with no counterpart
  line in the reference; what the entry's own comment states (dst = src + add * scale[row // rows_per_scale]; NCHW fp32 * scale
  -> NHWC rows, the batch repeated `rep` times; prev = k_x0 x0 + k_x x + k_eps eps + k_h hist + k_noise noise; ...).

`build(name)` makes the operands of a case on the CPU: every operand is a VIEW of a wider buffer of its own (spare rows and
columns hold NaN for inputs and SENT for outputs), and the GPU file copies each whole storage to the device and keeps the view.
`reference(name)` returns, per output tensor, a `Ref` over the WHOLE storage of that tensor as float64: `want`, `lo`, `hi`
(`value`, `slack` before the output rounding).  Where the launch writes nothing, want = lo = hi = what the buffer held, so one
comparison covers "inside the bound" and "nothing else written".  `standin(name, mut)` returns the same storages in the output's
own type, so that bits can be compared.  The stored 16-bit and fp32 inputs are exact.

The bound.  u = 2^-24 per fp32 operation, counted in the kernel's own order; the file is built with -ffp-contract=off, so every
multiply and every add rounds (no FMA).  Products of u-sized terms are covered by the factor 1 + 2^-9 on the slack (`SECOND`).
`lo` / `hi` are the images of value -+ slack under the output rounding (monotone), as in tests/norm_ref.py.
  sinusoid   x = ln(1e4) k / half.  The fp32 constant (u), c * k (u), / half (u): the argument of expf is off by 3 u x; expf,
             cosf and sinf of libm are ASSUMED within 1 ulp (2 u) -- the texts at hand give no figure and NOBODY MEASURED IT.
             rel(w) = 3 u x + 2 u, a = val * w (u): |d a| = |a| (3 x + 3) u, carried through |d cos|, |d sin| <= 1, plus 2 u for
             cosf / sinf themselves:  slack = |a| (3 x + 3) u + 2 u.
  silu       `silu_f`: x * rcp(1 + exp2(-log2e x)).  The constant (u) and the product (u) move the exponent by 2 u log2e |x|, i.e.
             e by a relative 2 u |x|; v_exp_f32 and v_rcp_f32 are ASSUMED within 1 ulp (2 u each), unmeasured as above.
             rel(1 + e) = rel(e) e / (1 + e) + u; rcp 2 u; the product u:
             slack = |silu| ((2 |x| + 2) e / (1 + e) + 4) u + |x| 2^-126      (the last term: a flushed v_exp / v_rcp result)
  copy_add   a * s (u), src + . (u):  slack = u (|a s| + |value|); without `add` the bits are copied, slack 0.
  pack       x * scale (u):  slack = u |value|.     unpack, transpose, copy_segments: exact, slack 0.
  lcm_step   p = sb e (u), s = x - p (u), x0 = s / sa (u), co x0 (u), cs x (u), the sum (u):
             e(x0) = u (|p| + |s|) / |sa| + u |x0|;  slack = |co| e(x0) + u (|co x0| + |cs x| + |den|).  Both outputs take the same
             fp32 value: the fp16 one rounds it again (covered by the image), the fp32 one is it.
  sched_step_f32 (with and without hist)   x0 as above with (sb, sa) = coef[1], coef[2]; pv = k_x0 x0 + k_x x (3 u), then each
             term that is not skipped adds u |term| + u |pv|.  prev, hist (= x0) and x0_out are outputs.
  axpby      a x (u), b y (u), the sum (u):  slack = u (|a x| + |b y| + |value|).
  blend      w = y / ext (u), 1 - w (u), two products, the sum:  slack = u (|a| (w + 2 (1 - w)) + 2 |b| w + |value|).
  rescale    per element, fp32: d = t - u_ (u), g d (u), u_ + g d (u): delta = u (2 |g d| + |e|); the PAG term q = t - p (u),
             s q (u), e + s q (u): delta += u (2 |s q| + |e'|).  t itself is exact.  The sums run in fp64 over the fp32 values:
             a thread adds C ceil(HW / 1024) terms, the butterfly 6, thread 0 the 16 waves: k = C ceil(HW / 1024) + 22,
             g64(k) = k 2^-53 / (1 - k 2^-53).  M2 = s2 - s1^2 / n moves, to first order in delta, by 2 sum |e - mean| delta
             (the perturbation enters both sums; their difference is exactly this), and by the accumulation and the one-pass
             cancellation  g64(k) (sum e^2 + 2 |mean| sum |e|) + 4 2^-53 s1^2 / n.  With rel = dM2 / M2 of the text and of the
             guided rows,  slack = phi ratio (rel_t + rel_c) / 2 + 8 2^-53 |value|  (division, sqrt, product, sum in fp64), then
             the one rounding to fp32.  `Ref.terms` holds |mean| / spread and each share per case: at a mean of 100 spreads the
             cancellation term is 1e4 g64(k) ~ 3e-12 of M2, far below the 1e-7 of the element roundings -- fp64 sums make the
             one-pass form harmless, and the bound says so.
No term comes from a kernel's output; no tolerance is a literal.

Bit classes.  Without a transcendental, IEEE arithmetic and contract-off make the stand-in's bits what a correct kernel stores:
copy_add, pack, unpack, lcm_step, transpose, copy_segments, blend, axpby, sched_step_f32 (`BIT_KINDS`).  torch CPU gives the
fp16 / bf16 roundings (nearest even, overflow to inf, subnormals kept).

Out of scope: offsets beyond 2 GiB; `njobs` near 65535; what iir_prefetch achieves (it has no output: the GPU file can show no
more than an OK status and an unchanged buffer).
"""
import collections
import functools
import math

import numpy as np
import torch

from norm_ref import F32, SECOND, U, _rng, rnd, tdtype

U64 = 2.0 ** -53
SENT = 7.0
SENT8 = 0x55
NAN = float("nan")
LN1E4_32 = F32(9.210340371976184)
LOG2E32 = F32(1.4426950408889634)
CH = 4                                   # latent channels of every NHWC <-> NCHW case

Ref = collections.namedtuple("Ref", "want lo hi value slack terms")
Case = collections.namedtuple("Case", "name kind opt")

BIT_KINDS = ("copy_add", "pack", "unpack", "lcm", "transpose", "segments", "blend", "axpby", "step")


def g64(k):
    return k * U64 / (1.0 - k * U64)


# ---- storages and views -----------------------------------------------------------------------------------------------------------
def flat(t):
    """The whole storage of t as a 1-D tensor of its type."""
    return torch.empty(0, dtype=t.dtype, device=t.device).set_(t.untyped_storage())


def like(view, base):
    """The view `view` describes, on the 1-D tensor `base` (a copy of its storage, any type)."""
    return torch.as_strided(base, tuple(view.shape), view.stride(), view.storage_offset())


def framed(t, ld=None, c0=0, fill=NAN):
    """A view holding the 2-D (or 1-D) tensor t inside a buffer with a spare row (1-D: 8 spare elements) before and after it and `ld`
    columns, the view starting at column c0."""
    if t.dim() == 1:
        buf = torch.full((t.numel() + 16,), fill, dtype=t.dtype)
        v = buf[8:8 + t.numel()]
    else:
        rows, cols = t.shape
        buf = torch.full((rows + 2, cols if ld is None else ld), fill, dtype=t.dtype)
        v = buf[1:1 + rows, c0:c0 + cols]
    v.copy_(t)
    return v


def framed_nd(t, fill):
    """t as the middle slices of a contiguous buffer with one more leading slice on either side."""
    buf = torch.full((t.shape[0] + 2,) + tuple(t.shape[1:]), fill, dtype=t.dtype)
    buf[1:-1] = t
    return buf[1:-1]


def _dt(t):
    return {torch.float16: "f16", torch.bfloat16: "bf16", torch.float32: "f32", torch.uint8: "u8"}[t.dtype]


def _round(x, dtype):
    if dtype in ("f16", "bf16"):
        return rnd(x, dtype)
    if dtype == "f32":
        with np.errstate(over="ignore"):
            return np.asarray(x, np.float64).astype(F32).astype(np.float64)
    return np.asarray(x, np.float64)


def _ref(out_view, written, value, slack, terms=None):
    """A Ref over the storage of `out_view`: `written` (a sub-view of it) takes value -+ slack, the rest keeps what it holds."""
    v = flat(out_view).double()
    s = torch.zeros_like(v)
    like(written, v).copy_(torch.as_tensor(np.asarray(value, np.float64)))
    like(written, s).copy_(torch.as_tensor(np.asarray(slack, np.float64) * SECOND))
    v, s, dt = v.numpy(), s.numpy(), _dt(out_view)
    return Ref(_round(v, dt), _round(v - s, dt), _round(v + s, dt), v, s, terms or {})


def _out(out_view, written, res):
    """The stand-in's storage of `out_view`, in its own type: `written` takes res (already rounded to that type's values)."""
    b = flat(out_view).clone()
    like(written, b).copy_(torch.as_tensor(res).to(b.dtype))
    return b


def to_t(x32, dtype):
    """fp32 numpy -> torch tensor of the element type, with the hardware conversion's rounding (torch CPU)."""
    t = torch.from_numpy(np.ascontiguousarray(x32, dtype=F32))
    return t if dtype == "f32" else t.to(tdtype(dtype))


def as64(t):
    t = t.detach().cpu()
    return (t.double() if t.dtype != torch.uint8 else t.to(torch.float64)).numpy()


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]).numpy()


# ---- sinusoid -----------------------------------------------------------------------------------------------------------------------
SIN_VALS = (0.0, 1.0, 999.0, 1024.0, 37.25, 512.0, 3.0, 250.5)


def _b_sinusoid(cs):
    o = cs.opt
    rows, nv, dim, off = o["rows"], o["n_vals"], o["dim"], o["col_off"]
    vals = torch.tensor([SIN_VALS[(3 * i + o.get("rot", 0)) % 8] for i in range(rows * nv)], dtype=torch.float32).reshape(rows, nv)
    width = off + nv * dim + 3                               # three columns after the last written one
    out = framed(torch.full((rows, width), SENT, dtype=torch.float16), ld=width + 7, c0=2, fill=SENT)
    return dict(vals=vals, out=out)


def _sin_written(cs, t):
    o = cs.opt
    return t["out"][:, o["col_off"]:o["col_off"] + o["n_vals"] * o["dim"]]


def _r_sinusoid(cs, t):
    o = cs.opt
    rows, nv, dim = o["rows"], o["n_vals"], o["dim"]
    half = dim // 2
    x = math.log(10000.0) * np.arange(half) / half
    ang = t["vals"].double().numpy()[:, :, None] * np.exp(-x)[None, None, :]
    value = np.concatenate([np.cos(ang), np.sin(ang)], -1).reshape(rows, nv * dim)
    s = np.abs(ang) * (3 * x + 3) * U + 2 * U
    slack = np.concatenate([s, s], -1).reshape(rows, nv * dim)
    return {"out": _ref(t["out"], _sin_written(cs, t), value, slack)}


def _f32(fn, x):
    return fn(np.asarray(x, np.float64)).astype(F32)


def _s_sinusoid(cs, t, mut):
    o = cs.opt
    rows, nv, dim = o["rows"], o["n_vals"], o["dim"]
    half = dim >> 1
    idx = np.arange(rows * nv * half)
    k, v, r = idx % half, (idx // half) % nv, idx // (half * nv)
    w = _f32(np.exp, (-LN1E4_32 * k.astype(F32)) / F32(dim if mut == "sin_k_over_dim" else half))
    a = t["vals"].numpy()[r, v] * w
    c, s = _f32(np.cos, a), _f32(np.sin, a)
    if mut == "sin_cos_swapped":
        c, s = s, c
    res = np.zeros((rows, nv * dim), F32)
    res[r, v * dim + k] = c
    res[r, v * dim + half + k] = s
    return {"out": _out(t["out"], _sin_written(cs, t), to_t(res, "f16"))}


# ---- silu ---------------------------------------------------------------------------------------------------------------------------
SILU_SPECIAL = (65504.0, -65504.0, 0.0, -0.0, 2.0 ** -24, -2.0 ** -24, 3.0e-5, -3.0e-5)


def _b_silu(cs):
    n = cs.opt["n"]
    x = np.concatenate([np.array(SILU_SPECIAL), np.linspace(-12.0, 12.0, n - 8)]) if n > 8 else np.array(SILU_SPECIAL)
    return dict(x=framed(to_t(x, "f16")), out=framed(torch.full((n,), SENT, dtype=torch.float16), fill=SENT))


def _r_silu(cs, t):
    x = t["x"].double().numpy()
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(-x)
        value = x / (1.0 + e)
        share = np.where(np.isfinite(e), e / (1.0 + e), 1.0)
    slack = np.abs(value) * ((2 * np.abs(x) + 2) * share + 4) * U + np.abs(x) * 2.0 ** -126
    return {"out": _ref(t["out"], t["out"], value, slack)}


def _s_silu(cs, t, mut):
    x = t["x"].float().numpy()
    with np.errstate(over="ignore", divide="ignore"):
        e = _f32(np.exp2, -LOG2E32 * x)
        res = x * (1.0 / (F32(1) + e).astype(np.float64)).astype(F32)
    w = t["out"][:-8] if mut == "silu_tail_dropped" else t["out"]
    return {"out": _out(t["out"], w, to_t(res[:w.numel()], "f16"))}


# ---- copy_add -----------------------------------------------------------------------------------------------------------------------
def _b_copy_add(cs):
    o = cs.opt
    M, C = o["M"], o["C"]
    rng = _rng(cs.name)
    src = (rng.standard_normal((M, C)) * 2).astype(F32)
    add = (rng.standard_normal((M, C)) * 2).astype(F32)
    src[0, 0], add[0, 0] = 60000.0, 60000.0                  # the sum leaves fp16
    src[M - 1, 1], add[M - 1, 1] = 2.0 ** -24, 0.0           # an fp16 subnormal stays one
    t = dict(src=framed(to_t(src, "f16"), ld=o["lds"], c0=8))
    width = o["dst_off"] + C
    t["dst"] = framed(torch.full((M, width), SENT, dtype=torch.float16), ld=o["ldd"], c0=8, fill=SENT)
    if o["add"]:
        t["add"] = framed(to_t(add, "f16"), ld=o["lda"], c0=16)
    if o["rps"]:
        ns = -(-M // o["rps"])
        t["scale"] = framed(torch.tensor([(0.5 + 0.37 * i) * (-1.0 if i % 3 == 2 else 1.0) for i in range(ns)], dtype=torch.float32))
    return t


def _ca_written(cs, t):
    return t["dst"][:, cs.opt["dst_off"]:]


def _ca_scale(cs, t, shift=0):
    o = cs.opt
    if not o["rps"]:
        return np.ones(o["M"])
    s = t["scale"].double().numpy()
    return s[np.minimum((np.arange(o["M"]) + shift) // o["rps"], s.size - 1)]


def _r_copy_add(cs, t):
    src = t["src"].double().numpy()
    if not cs.opt["add"]:
        return {"dst": _ref(t["dst"], _ca_written(cs, t), src, np.zeros_like(src))}
    p = t["add"].double().numpy() * _ca_scale(cs, t)[:, None]
    value = src + p
    return {"dst": _ref(t["dst"], _ca_written(cs, t), value, U * (np.abs(p) + np.abs(value)))}


def _s_copy_add(cs, t, mut):
    o = cs.opt
    if not o["add"]:
        return {"dst": _out(t["dst"], _ca_written(cs, t), t["src"])}
    s = _ca_scale(cs, t, 1 if mut == "ca_scale_index_m_plus_1" else 0).astype(F32)
    if mut == "ca_add_scale_ignored":
        s = np.ones_like(s)
    with np.errstate(over="ignore"):
        res = t["src"].float().numpy() + t["add"].float().numpy() * s[:, None]
    return {"dst": _out(t["dst"], _ca_written(cs, t), to_t(res, "f16"))}


# ---- pack / unpack ------------------------------------------------------------------------------------------------------------------
PACK_SCALES = {"s1": 1.0, "s0862": 0.0862, "big": 3.0e4}


def _b_pack(cs):
    o = cs.opt
    B, C, H, W = o["shape"]
    x = (_rng(f"pack{o['shape']}").standard_normal((B, C, H, W)) * 3).astype(F32)
    x.reshape(-1)[::5] *= F32(1e-9)                          # with the big scale: products inside the fp16 subnormals
    rows = o["rep"] * B * H * W
    out = framed(torch.full((rows, C), SENT, dtype=tdtype(o["dtype"])), ld=o["ld"], fill=SENT)
    return dict(x=torch.from_numpy(x), out=out, scale=torch.tensor([PACK_SCALES[o["scale"]]], dtype=torch.float32))


def _r_pack(cs, t):
    o = cs.opt
    B, C, H, W = o["shape"]
    v = (t["x"].double() * t["scale"].double()).permute(0, 2, 3, 1).reshape(B * H * W, C).numpy()
    value = np.tile(v, (o["rep"], 1))
    return {"out": _ref(t["out"], t["out"], value, U * np.abs(value))}


def _s_pack(cs, t, mut):
    o = cs.opt
    B, C, H, W = o["shape"]
    HW, rep = H * W, o["rep"]
    x = t["x"].numpy().reshape(B, C, HW)
    with np.errstate(over="ignore"):
        v = to_t(x * t["scale"].numpy()[0], o["dtype"])                  # (B, C, HW)
    res = torch.zeros(rep * B * HW, C, dtype=v.dtype)
    b, p = np.divmod(np.arange(B * HW), HW)
    for k in range(rep):
        row = (b * rep + k if mut == "pack_row_b_rep_k" else k * B + b) * HW + p
        res[torch.from_numpy(row)] = v[torch.from_numpy(b), :, torch.from_numpy(p)]
    return {"out": _out(t["out"], t["out"], res)}


UNPACK_SPECIAL = (65504.0, -65504.0, -0.0, 2.0 ** -24, -3.0e-5, 1.0)


def _b_unpack(cs):
    o = cs.opt
    R, C, H, W = o["shape"]
    v = (_rng(f"unpack{o['shape']}").standard_normal((R * H * W, C)) * 3).astype(F32)
    v.reshape(-1)[:min(v.size, 6)] = UNPACK_SPECIAL[:min(v.size, 6)]
    return dict(x=framed(to_t(v, o["dtype"]), ld=o["ld"]), out=framed_nd(torch.full((R, C, H, W), SENT, dtype=torch.float32), SENT))


def _r_unpack(cs, t):
    R, C, H, W = cs.opt["shape"]
    value = t["x"].double().reshape(R, H, W, C).permute(0, 3, 1, 2).numpy()
    return {"out": _ref(t["out"], t["out"], value, np.zeros_like(value))}


def _s_unpack(cs, t, mut):
    R, C, H, W = cs.opt["shape"]
    HW = H * W
    x = t["x"].float().reshape(R, HW, C)
    res = torch.zeros(R * C * HW)
    r, p, c = np.meshgrid(np.arange(R), np.arange(HW), np.arange(C), indexing="ij")
    at = (r * HW + p) * C + c if mut == "unpack_pixel_channel_swapped" else (r * C + c) * HW + p
    res[torch.from_numpy(at.reshape(-1))] = x.reshape(-1)
    return {"out": _out(t["out"], t["out"], res.reshape(R, C, H, W))}


# ---- rescale_noise_cfg --------------------------------------------------------------------------------------------------------------
RS_G = 7.5
RS_LDE = 8


def _b_rescale(cs):
    o = cs.opt
    B, (H, W) = o["B"], o["hw"]
    HW = H * W
    rng = _rng(f"rs{B}x{HW}{o['mode']}")
    img = np.arange(B)[:, None, None]
    u = rng.standard_normal((B, HW, CH)) * (0.6 + 0.3 * img) + 0.1 * img
    tt = u * 0.7 + rng.standard_normal((B, HW, CH)) * (0.5 + 0.2 * img) + 0.05 * (np.arange(HW) % 9)[None, :, None]
    pp = tt + rng.standard_normal((B, HW, CH)) * 0.3
    if o["mode"] == "lm100":                                 # a mean of 100 spreads: where the one-pass variance is weakest
        u, tt, pp = u * 0.5 + 50.0, tt * 0.5 + 50.0, pp * 0.5 + 50.0
    pag = o["pag"]
    if pag is None or pag == 0.0:
        pp = np.full_like(pp, np.nan)                        # rows [2B, 3B) must not be read
    e = np.concatenate([u, tt, pp]).reshape(3 * B * HW, CH).astype(F32)
    coef = torch.full((8,), NAN, dtype=torch.float32)
    coef[0] = RS_G
    t = dict(eps=framed(to_t(e, "f16"), ld=RS_LDE), coef=coef, x=torch.zeros(B, CH, H, W),
             factor=framed(torch.full((B,), SENT, dtype=torch.float32), fill=SENT))
    if pag is not None:
        t["pag_s"] = torch.tensor([pag], dtype=torch.float32)
    return t


def _rs_rows(cs, t, dtype):
    B, (H, W) = cs.opt["B"], cs.opt["hw"]
    e = t["eps"].to(dtype).numpy().reshape(3, B, H * W, CH)
    return e[0], e[1], e[2]


def _r_rescale(cs, t):
    o = cs.opt
    B, (H, W) = o["B"], o["hw"]
    HW, n = H * W, CH * H * W
    u, tt, pp = _rs_rows(cs, t, torch.float64)
    g = float(t["coef"][0])
    s = float(t["pag_s"][0]) if "pag_s" in t else 0.0
    phi = float(F32(o["phi"]))
    gd = g * (tt - u)
    e = u + gd
    delta = U * (2 * np.abs(gd) + np.abs(e))
    if s != 0.0:
        sq = s * (tt - pp)
        e = e + sq
        delta = delta + U * (2 * np.abs(sq) + np.abs(e))
    ax = (1, 2)
    ratio = tt.std(axis=ax, ddof=1) / e.std(axis=ax, ddof=1)
    value = phi * ratio + (1.0 - phi)
    k = CH * -(-HW // 1024) + 22

    def acc(v):
        return g64(k) * ((v * v).sum(ax) + 2 * np.abs(v.mean(ax)) * np.abs(v).sum(ax)) + 4 * U64 * v.sum(ax) ** 2 / n

    m2 = lambda v: ((v - v.mean(ax, keepdims=True)) ** 2).sum(ax)
    rel_elem = 2 * (np.abs(e - e.mean(ax, keepdims=True)) * delta).sum(ax) / m2(e)
    rel_c, rel_t = acc(e) / m2(e), acc(tt) / m2(tt)
    slack = phi * ratio * 0.5 * (rel_elem + rel_c + rel_t) + 8 * U64 * np.abs(value)
    terms = dict(mean_over_spread=float((np.abs(tt.mean(ax)) / tt.std(axis=ax)).max()), rel_elem=float(rel_elem.max()),
                 rel_acc_cfg=float(rel_c.max()), rel_acc_text=float(rel_t.max()), chain=k)
    return {"factor": _ref(t["factor"], t["factor"], value, slack, terms)}


def _s_rescale(cs, t, mut):
    o = cs.opt
    u, tt, pp = _rs_rows(cs, t, torch.float32)
    g = t["coef"].numpy()[0]
    ps = t["pag_s"].numpy()[0] if "pag_s" in t else F32(0)
    e = u + g * (tt - u)
    if ps != 0:
        q = ps * (tt - pp)
        e = e - q if mut == "rs_pag_sign" else e + q
    dev = u if mut == "rs_uncond_dev" else tt
    if mut == "rs_drop_p1024":
        e, dev = e[:, :1024], dev[:, :1024]
    n = float(CH * o["hw"][0] * o["hw"][1])

    def var(v):
        v = v.astype(np.float64)
        s1, s2 = v.sum((1, 2)), (v * v).sum((1, 2))
        return (s2 - s1 * s1 / n) / (n - 1.0)

    phi = float(F32(o["phi"]))
    res = (phi * np.sqrt(var(dev) / var(e)) + (1.0 - phi)).astype(F32)
    return {"factor": _out(t["factor"], t["factor"], res)}


# ---- lcm_step -----------------------------------------------------------------------------------------------------------------------
LCM_COEF = (0.6, 0.8, 0.95, 0.05)                                        # sqrt_beta, sqrt_alpha, c_out, c_skip


def _b_lcm(cs):
    o = cs.opt
    B, rep, (H, W) = o["B"], o["rep"], o["hw"]
    Rr, HW = B * rep, H * W
    rng = _rng(cs.name)
    x = (rng.standard_normal((B, CH, H, W)) * (1.0 + np.arange(B))[:, None, None, None] + np.arange(B)[:, None, None, None]).astype(F32)
    e = rng.standard_normal((Rr * HW, CH)).astype(F32)
    t = dict(eps=framed(to_t(e, "f16"), ld=o["lde"]), x=torch.from_numpy(x), coef=torch.tensor(LCM_COEF, dtype=torch.float32),
             out=framed(torch.full((Rr * HW, CH), SENT, dtype=torch.float16), ld=o["ldo"], fill=SENT))
    if o["nchw"]:
        t["out_nchw"] = framed_nd(torch.full((Rr, CH, H, W), SENT, dtype=torch.float32), SENT)
    return t


def _step_x0(xv, e, sb, sa):
    """x0 = (x - sb e) / sa and its fp32 error, per element (float64 arrays)."""
    p = sb * e
    s = xv - p
    x0 = s / sa
    return x0, U * (np.abs(p) + np.abs(s)) / abs(sa) + U * np.abs(x0)


def _r_lcm(cs, t):
    o = cs.opt
    B, rep, (H, W) = o["B"], o["rep"], o["hw"]
    Rr = B * rep
    sb, sa, co, csk = (float(v) for v in t["coef"].double())
    sample = t["x"].double().repeat(rep, 1, 1, 1).numpy()                      # cat([latents] * rep)
    eps = t["eps"].double().reshape(Rr, H, W, CH).permute(0, 3, 1, 2).numpy()
    x0, e0 = _step_x0(sample, eps, sb, sa)
    den = co * x0 + csk * sample
    slack = abs(co) * e0 + U * (np.abs(co * x0) + np.abs(csk * sample) + np.abs(den))
    nhwc = lambda a: a.transpose(0, 2, 3, 1).reshape(Rr * H * W, CH)
    out = {"out": _ref(t["out"], t["out"], nhwc(den), nhwc(slack))}
    if o["nchw"]:
        out["out_nchw"] = _ref(t["out_nchw"], t["out_nchw"], den, slack)
    return out


def _s_lcm(cs, t, mut):
    o = cs.opt
    B, rep, (H, W) = o["B"], o["rep"], o["hw"]
    Rr, HW = B * rep, H * W
    sb, sa, co, csk = t["coef"].numpy()
    x = t["x"].numpy().reshape(B, CH, HW)
    i = np.arange(Rr * HW)
    r, p = i // HW, i % HW
    b = r // rep if mut == "lcm_image_r_div_rep" else r % B
    xv = x[b, :, p]                                                            # (R HW, C)
    e = t["eps"].float().numpy()
    x0 = (xv - sb * e) / sa
    d = co * x0 + csk * xv
    out = {"out": _out(t["out"], t["out"], to_t(d, "f16"))}
    if o["nchw"]:
        out["out_nchw"] = _out(t["out_nchw"], t["out_nchw"], torch.from_numpy(d.reshape(Rr, HW, CH).transpose(0, 2, 1).reshape(Rr, CH, H, W).copy()))
    return out


# ---- transpose ----------------------------------------------------------------------------------------------------------------------
def _b_transpose(cs):
    rows, cols, pad = cs.opt["shape"]
    v = (_rng(cs.name).standard_normal((rows, cols)) + 0.25 * (1 + np.arange(rows) % 5)[:, None]).astype(F32)
    # the engine's form: the source a column slice kvb[:, inner:], the destination the second window of a wider vt
    return dict(x=framed(to_t(v, "f16"), ld=cols + 24, c0=8),
                out=framed(torch.full((cols, pad), SENT, dtype=torch.float16), ld=2 * pad + 8, c0=pad, fill=SENT))


def _r_transpose(cs, t):
    rows, cols, pad = cs.opt["shape"]
    value = np.zeros((cols, pad))
    value[:, :rows] = t["x"].double().numpy().T
    return {"out": _ref(t["out"], t["out"], value, np.zeros_like(value))}


def _s_transpose(cs, t, mut):
    rows, cols, pad = cs.opt["shape"]
    x = t["x"]
    res = torch.zeros(cols, pad, dtype=torch.float16)
    for by in range(0, pad, 32):                                               # one 32 x 32 tile of the kernel at a time
        for bx in range(0, cols, 32):
            r = torch.arange(by, by + 32)
            c = torch.arange(bx, bx + 32)
            tile = x[r.clamp(max=rows - 1)][:, c.clamp(max=cols - 1)].clone()
            if mut != "tr_clamp_last_tile":
                tile[r >= rows] = 0
                tile[:, c >= cols] = 0
            rr, cc = r[r < pad], c[c < cols]
            res[bx:bx + cc.numel(), by:by + rr.numel()] = tile[:rr.numel(), :cc.numel()].T
    w = t["out"][:, :rows] if mut == "tr_no_zero_fill" else t["out"]
    return {"out": _out(t["out"], w, res[:, :w.shape[1]])}


# ---- copy_segments ------------------------------------------------------------------------------------------------------------------
def _b_segments(cs):
    t = {}
    for j, units in enumerate(cs.opt["units"]):
        g = torch.Generator().manual_seed(1000 + j + units)
        src = torch.randint(0, 256, (units * 16,), dtype=torch.uint8, generator=g)
        sb = torch.full((units * 16 + 32,), 0xAA, dtype=torch.uint8)
        sb[16:-16] = src
        t[f"src{j}"] = sb[16:-16]
        t[f"dst{j}"] = torch.full((units * 16 + 32,), SENT8, dtype=torch.uint8)[16:-16]          # sentinel bytes on both sides
    return t


def _r_segments(cs, t):
    out = {}
    for j in range(len(cs.opt["units"])):
        v = as64(t[f"src{j}"])
        out[f"dst{j}"] = _ref(t[f"dst{j}"], t[f"dst{j}"], v, np.zeros_like(v))
    return out


def _s_segments(cs, t, mut):
    out = {}
    mx = max(cs.opt["units"]) * 16
    for j in range(len(cs.opt["units"])):
        d = flat(t[f"dst{j}"]).clone()
        s = flat(t[f"src{j}"])
        n = min(mx, d.numel() - 16) if mut == "cs_max_units_for_every_job" else t[f"src{j}"].numel()
        d[16:16 + n] = s[16:16 + n]                          # (the mutant runs on into whatever follows, here the frame)
        out[f"dst{j}"] = d
    return out


# ---- blend_tiles --------------------------------------------------------------------------------------------------------------------
BLEND_PLANES = (2, 3)                                                          # 6 planes


def _b_blend(cs):
    o = cs.opt
    rng = _rng(cs.name)
    mk = lambda H, W, fill: framed_nd(torch.from_numpy(rng.standard_normal(BLEND_PLANES + (H, W)).astype(F32) * 2 + 1), fill)
    return dict(a=mk(o["Ha"], o["Wa"], SENT), b=mk(o["Hb"], o["Wb"], SENT))          # `a` is checked too: it must come back untouched


def _bl_geo(o):
    ext = o["ext"]
    return (ext, min(o["Wa"], o["Wb"])) if o["vertical"] else (min(o["Ha"], o["Hb"]), ext)


def _r_blend(cs, t):
    o = cs.opt
    ext = o["ext"]
    rows, cols = _bl_geo(o)
    a, b = t["a"].double().numpy(), t["b"].double().numpy()
    if o["vertical"]:
        av, w = a[:, :, o["Ha"] - ext:, :cols], (np.arange(ext) / ext)[:, None]
    else:
        av, w = a[:, :, :rows, o["Wa"] - ext:], (np.arange(ext) / ext)[None, :]
    bv = b[:, :, :rows, :cols]
    value = av * (1 - w) + bv * w
    slack = U * (np.abs(av) * (w + 2 * (1 - w)) + 2 * np.abs(bv) * w + np.abs(value))
    za = np.zeros_like(a)
    return {"b": _ref(t["b"], t["b"][:, :, :rows, :cols], value, slack), "a": _ref(t["a"], t["a"], a, za)}


def _s_blend(cs, t, mut):
    o = cs.opt
    ext, Ha, Wa, Hb, Wb, vert = o["ext"], o["Ha"], o["Wa"], o["Hb"], o["Wb"], o["vertical"]
    rows, cols = _bl_geo(o)
    if mut == "bl_h_clip_hb" and not vert:
        rows = Hb
    planes = BLEND_PLANES[0] * BLEND_PLANES[1]
    af, bf = flat(t["a"]).numpy(), flat(t["b"]).clone().numpy()
    a0, b0 = t["a"].storage_offset(), t["b"].storage_offset()
    i = np.arange(planes * rows * cols)
    x, y, p = i % cols, (i // cols) % rows, i // (cols * rows)
    with np.errstate(divide="ignore", invalid="ignore"):
        w = (y if vert else x).astype(F32) / F32(ext - 1 if mut == "bl_w_ext_minus_1" else ext)
        ya = y if (mut == "bl_a_row_y" or not vert) else Ha - ext + y
        xa = x if vert else Wa - ext + x
        av = af[np.minimum(a0 + (p * Ha + ya) * Wa + xa, af.size - 1)]          # (the clip mutant reads past the plane: clamped here)
        bi = b0 + (p * Hb + y) * Wb + x
        bf[bi] = av * (F32(1) - w) + bf[bi] * w
    return {"b": torch.from_numpy(bf), "a": flat(t["a"]).clone()}


# ---- axpby, sched_step_f32, sched_step_hist_f32 -------------------------------------------------------------------------------------
def _vec(rng, n, fill=NAN, scale=1.0):
    return framed(torch.from_numpy((rng.standard_normal(n) * scale).astype(F32)), fill=fill)


def _b_axpby(cs):
    n = cs.opt["n"]
    rng = _rng(cs.name)
    return dict(x=_vec(rng, n), y=_vec(rng, n, scale=3.0), coef=torch.tensor([0.8366, -0.5477], dtype=torch.float32),
                out=framed(torch.full((n,), SENT, dtype=torch.float32), fill=SENT))


def _r_axpby(cs, t):
    a, b = (float(v) for v in t["coef"].double())
    ax, by = a * t["x"].double().numpy(), b * t["y"].double().numpy()
    return {"out": _ref(t["out"], t["out"], ax + by, U * (np.abs(ax) + np.abs(by) + np.abs(ax + by)))}


def _s_axpby(cs, t, mut):
    a, b = t["coef"].numpy()[::-1] if mut == "axpby_coef_swapped" else t["coef"].numpy()
    return {"out": _out(t["out"], t["out"], torch.from_numpy(a * t["x"].numpy() + b * t["y"].numpy()))}


STEP_COEF = {"full": (NAN, 0.6, 0.8, 0.35, 0.55, -0.2, 0.3, 0.45),           # {_, sb, sa, k_x0, k_x, k_eps, k_noise, k_h}
             "zero": (NAN, 0.6, 0.8, 0.35, 0.55, 0.0, 0.0, 0.0)}


def _b_step(cs):
    o = cs.opt
    n = o["n"]
    rng = _rng(cs.name)
    skip = o["coef"] == "zero"                               # a zero coefficient with NaN in the plane it skips
    t = dict(eps=_vec(rng, n), x=_vec(rng, n, scale=2.0), coef=torch.tensor(STEP_COEF[o["coef"]], dtype=torch.float32),
             prev=framed(torch.full((n,), SENT, dtype=torch.float32), fill=SENT))
    if o["noise"]:
        t["noise"] = framed(torch.full((n,), NAN, dtype=torch.float32)) if skip else _vec(rng, n)
    if o["x0"]:
        t["x0_out"] = framed(torch.full((n,), SENT, dtype=torch.float32), fill=SENT)
    if o["hist"]:
        t["hist"] = framed(torch.full((n,), NAN, dtype=torch.float32), fill=SENT) if skip else _vec(rng, n, fill=SENT)
    return t


def _r_step(cs, t):
    o = cs.opt
    k = [float(v) for v in t["coef"].double()]
    xv, e = t["x"].double().numpy(), t["eps"].double().numpy()
    x0, e0 = _step_x0(xv, e, k[1], k[2])
    pv = k[3] * x0 + k[4] * xv
    slack = abs(k[3]) * e0 + U * (np.abs(k[3] * x0) + np.abs(k[4] * xv) + np.abs(pv))
    terms = [(k[5], e)]
    if o["hist"]:
        terms.append((k[7], t["hist"].double().numpy()))
    if o["noise"]:
        terms.append((k[6], t["noise"].double().numpy()))
    for c, plane in terms:
        if c != 0.0:
            pv = pv + c * plane
            slack = slack + U * (np.abs(c * plane) + np.abs(pv))
    out = {"prev": _ref(t["prev"], t["prev"], pv, slack)}
    for name in ("hist", "x0_out"):
        if name in t:
            out[name] = _ref(t[name], t[name], x0, e0)
    return out


def _s_step(cs, t, mut):
    o = cs.opt
    k = t["coef"].numpy()
    kn, kh = (k[7], k[6]) if mut == "st_kh_kn_swapped" else (k[6], k[7])
    xv, e = t["x"].numpy(), t["eps"].numpy()
    x0 = (xv - k[1] * e) / k[2]
    pv = k[3] * x0 + k[4] * xv
    if k[5] != 0:
        pv = pv + k[5] * e
    if o["hist"] and kh != 0:
        pv = pv + kh * t["hist"].numpy()
    if o["noise"] and kn != 0:
        pv = pv + kn * t["noise"].numpy()
    out = {"prev": _out(t["prev"], t["prev"], torch.from_numpy(pv))}
    for name in ("hist", "x0_out"):
        if name in t:
            out[name] = _out(t[name], t[name], torch.from_numpy(x0))
    return out


# ---- the table ----------------------------------------------------------------------------------------------------------------------
_KINDS = {"sinusoid": (_b_sinusoid, _r_sinusoid, _s_sinusoid), "silu": (_b_silu, _r_silu, _s_silu),
          "copy_add": (_b_copy_add, _r_copy_add, _s_copy_add), "pack": (_b_pack, _r_pack, _s_pack),
          "unpack": (_b_unpack, _r_unpack, _s_unpack), "rescale": (_b_rescale, _r_rescale, _s_rescale), "lcm": (_b_lcm, _r_lcm, _s_lcm),
          "transpose": (_b_transpose, _r_transpose, _s_transpose), "segments": (_b_segments, _r_segments, _s_segments),
          "blend": (_b_blend, _r_blend, _s_blend), "axpby": (_b_axpby, _r_axpby, _s_axpby), "step": (_b_step, _r_step, _s_step)}

MUTANTS = {"sinusoid": ("sin_cos_swapped", "sin_k_over_dim"), "silu": ("silu_tail_dropped",),
           "copy_add": ("ca_scale_index_m_plus_1", "ca_add_scale_ignored"), "pack": ("pack_row_b_rep_k",),
           "unpack": ("unpack_pixel_channel_swapped",), "rescale": ("rs_uncond_dev", "rs_pag_sign", "rs_drop_p1024"),
           "lcm": ("lcm_image_r_div_rep",), "transpose": ("tr_no_zero_fill", "tr_clamp_last_tile"),
           "segments": ("cs_max_units_for_every_job",), "blend": ("bl_w_ext_minus_1", "bl_a_row_y", "bl_h_clip_hb"),
           "axpby": ("axpby_coef_swapped",), "step": ("st_kh_kn_swapped",)}

SEG_GRID_UNITS = 256 * 1024 + 37                              # the fixed-grid form, 37 threads with a second trip


def _cases():
    out = []

    def add(name, kind, **opt):
        out.append(Case(name, kind, opt))

    add("sin.one", "sinusoid", rows=1, n_vals=1, dim=2, col_off=0, rot=1)                 # 1 thread
    add("sin.192", "sinusoid", rows=2, n_vals=3, dim=64, col_off=8)                       # one partial block
    add("sin.time_ids", "sinusoid", rows=3, n_vals=6, dim=256, col_off=1280)              # the engine's form: 9 whole blocks
    add("sin.270", "sinusoid", rows=3, n_vals=5, dim=36, col_off=5, rot=2)                # 270 threads: a second, partial block
    add("sin.timestep", "sinusoid", rows=3, n_vals=1, dim=320, col_off=0, rot=2)          # 480 threads
    for n in (8, 1000, 2048 + 8):
        add(f"silu.n{n}", "silu", n=n)
    ca = dict(add=True, rps=0, lds=32, lda=48, ldd=64, dst_off=16)
    add("ca.noadd", "copy_add", M=5, C=8, add=False, rps=0, lds=24, lda=0, ldd=32, dst_off=0)
    add("ca.noscale", "copy_add", M=37, C=24, **ca)
    add("ca.rps1", "copy_add", M=37, C=24, **dict(ca, rps=1))
    add("ca.rps35", "copy_add", M=100, C=24, **dict(ca, rps=35))                          # 300 chunks: a block ends inside row 85
    add("ca.rpsM", "copy_add", M=37, C=24, **dict(ca, rps=37, dst_off=0))
    add("ca.c8", "copy_add", M=300, C=8, **dict(ca, rps=35))
    add("ca.c2560", "copy_add", M=3, C=2560, add=True, rps=2, lds=2568, lda=2584, ldd=2600, dst_off=8)
    for shape, rep, ld, dt, sc, dev in (((1, 4, 1, 1), 1, 4, "f16", "s1", False), ((2, 4, 5, 7), 2, 8, "f16", "s0862", False),
                                        ((2, 4, 5, 7), 2, 8, "f16", "s0862", True), ((3, 4, 16, 17), 3, 8, "bf16", "s0862", True),
                                        ((3, 4, 16, 17), 3, 4, "f16", "big", False), ((2, 4, 5, 7), 1, 4, "bf16", "big", True),
                                        ((3, 4, 16, 17), 1, 8, "bf16", "s1", False), ((2, 4, 5, 7), 3, 8, "f16", "big", True)):
        add(f"pack.{'x'.join(map(str, shape))}.r{rep}.ld{ld}.{dt}.{sc}.{'dev' if dev else 'host'}", "pack", shape=shape, rep=rep, ld=ld,
            dtype=dt, scale=sc, dscale=dev)
    for shape, ld, dt in (((1, 4, 1, 1), 4, "f16"), ((2, 4, 5, 7), 8, "f16"), ((3, 4, 16, 17), 8, "bf16"), ((3, 4, 16, 17), 4, "f16"),
                          ((2, 4, 5, 7), 4, "bf16")):
        add(f"unpack.{'x'.join(map(str, shape))}.ld{ld}.{dt}", "unpack", shape=shape, ld=ld, dtype=dt)
    for B, hw, pag, phi, mode in ((1, (5, 7), None, 0.7, "c"), (3, (32, 32), None, 0.7, "c"), (3, (25, 41), None, 1.0, "c"),
                                  (3, (33, 67), None, 0.7, "c"), (3, (33, 67), 0.0, 0.7, "c"), (3, (33, 67), 2.75, 0.7, "c"),
                                  (1, (25, 41), 2.75, 0.0, "c"), (3, (33, 67), None, 0.7, "lm100"), (1, (5, 7), 2.75, 1.0, "c"),
                                  (3, (25, 41), 2.75, 1.0, "lm100")):
        tag = "plain" if pag is None else f"pag{pag:g}"
        add(f"rs.b{B}.hw{hw[0] * hw[1]}.{tag}.phi{phi:g}" + ("" if mode == "c" else "." + mode), "rescale", B=B, hw=hw, pag=pag, phi=phi,
            mode=mode)
    for B, rep, hw, nchw in ((2, 1, (5, 7), True), (2, 2, (9, 33), True), (3, 2, (5, 7), False), (3, 1, (9, 33), False), (3, 2, (9, 33), True)):
        add(f"lcm.b{B}.r{rep}.hw{hw[0] * hw[1]}.{'nchw' if nchw else 'nhwc'}", "lcm", B=B, rep=rep, hw=hw, nchw=nchw, lde=8, ldo=16)
    for shape in ((77, 64, 80), (1, 8, 8), (33, 33, 40), (32, 32, 32), (40, 64, 48), (257, 40, 264)):
        add("tr.%dx%d.p%d" % shape, "transpose", shape=shape)
    add("seg.one", "segments", units=(1,))
    add("seg.three", "segments", units=(1, 4097, 300))
    add("seg.grid", "segments", units=(SEG_GRID_UNITS, 5))
    for name, v, Ha, Wa, Hb, Wb, ext in (("v.same.e7", 1, 9, 11, 9, 11, 7), ("v.wa_gt_wb.e1", 1, 9, 13, 8, 11, 1), ("v.wa_lt_wb.full", 1, 5, 9, 7, 12, 5),
                                         ("h.same.e7", 0, 9, 11, 9, 11, 7), ("h.ha_gt_hb.e1", 0, 10, 11, 8, 12, 1), ("h.ha_lt_hb.full", 0, 6, 7, 9, 5, 5),
                                         ("h.ha_lt_hb.e7", 0, 6, 9, 9, 11, 7)):
        add("bl." + name, "blend", vertical=bool(v), Ha=Ha, Wa=Wa, Hb=Hb, Wb=Wb, ext=ext)
    for n in (1, 255, 257, 70):
        add(f"axpby.n{n}", "axpby", n=n)
    for n, noise, x0, coef in ((1, False, False, "full"), (255, True, True, "full"), (257, True, False, "full"), (70, False, True, "full"),
                               (257, True, True, "zero")):
        add(f"st.n{n}{'.noise' if noise else ''}{'.x0' if x0 else ''}.{coef}", "step", n=n, noise=noise, x0=x0, hist=False, coef=coef)
        add(f"sh.n{n}{'.noise' if noise else ''}{'.x0' if x0 else ''}.{coef}", "step", n=n, noise=noise, x0=x0, hist=True, coef=coef)
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return {c.name: c for c in out}


CASES = _cases()
PREFETCH_CASES = tuple((nbytes, blocks) for nbytes in (100, 128 * 1000 + 60) for blocks in (1, 32))


@functools.lru_cache(maxsize=None)
def build(name):
    """The operands of a case (CPU tensors, views of wider buffers).  Shared: leave them unchanged."""
    cs = CASES[name]
    return _KINDS[cs.kind][0](cs)


@functools.lru_cache(maxsize=None)
def reference(name):
    cs = CASES[name]
    return _KINDS[cs.kind][1](cs, build(name))


def standin(name, mut=None):
    cs = CASES[name]
    assert mut is None or mut in MUTANTS[cs.kind], (name, mut)
    return _KINDS[cs.kind][2](cs, build(name), mut)


def compare(got, ref):
    """(elements outside [lo, hi] or NaN, the worst |got - want| / bound: inf where the bound is 0 and the error is not)."""
    got = np.asarray(got, np.float64)
    bad = ~((got >= ref.lo) & (got <= ref.hi))
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(got - ref.want)
        err = np.where(got == ref.want, 0.0, np.where(np.isnan(err), np.inf, err))
        bound = np.maximum(np.where(ref.hi == ref.want, 0.0, ref.hi - ref.want), np.where(ref.lo == ref.want, 0.0, ref.want - ref.lo))
        ratio = np.where(err > 0, err / bound, 0.0)
        ratio = np.where(np.isnan(ratio), np.inf, ratio)
    return int(bad.sum()), float(ratio.max()) if ratio.size else 0.0


def worst(got, ref):
    got = np.asarray(got, np.float64)
    bad = np.flatnonzero(~((got >= ref.lo) & (got <= ref.hi)))
    i = int(bad[0]) if bad.size else 0
    return dict(at=i, outside=int(bad.size), got=float(got[i]), want=float(ref.want[i]), lo=float(ref.lo[i]), hi=float(ref.hi[i]))
