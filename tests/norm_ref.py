"""fp64 restatement of every launch of csrc/norm.hip (`ops.groupnorm` in the three-launch and the `partials=` form, `ops.layernorm`
plain / adaLN / transposed / fp8 out, `ops.adaln_batch`, `ops.softmax_rows`, `ops.softmax_rows_f32`), with a per-element bound
derived from the number formats and the kernels' own operation counts, the numpy fp32 stand-ins of the kernels, and the case table
of tests/test_norm_every_shape_gpu.py.  Plain helper for that file and for tests/test_norm_ref_cpu.py; no GPU use.

`reference(case)` returns a `Ref` in the layout of the output view, float64: `want`, `lo`, `hi`, `bound = max(hi - want,
want - lo)`, and `value`, `slack` (before the output rounding).  The stored 16-bit / fp32 inputs are exact.

Rounding points of the reference (the ones csrc/norm.hip documents, no others)
  GroupNorm  mean and biased variance of the stored values per (image, group) in fp64; a = rstd * gamma, b = beta - mean * a,
             x * a + b, optional SiLU, ONE rounding to fp16 / bf16.  `partials=`: the fp32 (mean, M2) per (64-row slab, channel)
             are inputs (built in fp64 from the stored x, rounded to fp32); mean = average of the means, M2 = sum M2 + 64 sum d^2.
  LayerNorm  (x - mean) * rstd, * gamma, + beta, * (1 + scale) + shift in the kernel's order, one rounding to fp16; fp8 out: that
             fp16 value to E4M3 (round to nearest even, saturating: `to_e4m3` of the GEMM reference).
  softmax    maximum subtracted, exp and sum, one rounding to fp16 / bf16.

The bound.  u = 2^-24 per fp32 operation, g(k) = k u / (1 - k u) for a chain of k of them.  The kernels are built without
-ffp-contract=off: a multiply-add may or may not be fused, and a fused one has one rounding fewer, so counting every multiply
and every add covers both.  v_exp_f32, v_rcp_f32 and v_rsq_f32 are ASSUMED to be within 1 ulp of fp32 (2 u); the texts at hand
give no figure and NOBODY MEASURED IT (tests/attention_ref.py makes the same assumption).  The error of rstd is carried exactly
(r / (2 (1 - r)), r < 2^-5 asserted); the products of the remaining u-sized terms with each other and with it are covered by a
factor 1 + 2^-9 on the slack.

GroupNorm, three launches.  Per (image, group): N samples, mean mu, variance var, sigma = sqrt(var), A = max |x|,
D = max |x - mu| (so any two partial means differ by <= 2 D, and a thread's samples lie within 2 D of its first one).
  thread      cnt samples about the first one: f = x - k0 (u |f|), s = sum f, q = sum f^2.
              |mean_t - exact| <= (g(cnt) + 2 u) 2 D + u A;   |M2_t - exact| <= (3 g(cnt) + 8 u) cnt (2 D)^2
  chan_merge  d = mb - mean, mean += d * (nb / tot): the error of the inputs does not grow ((1 - w) e_a + w e_b <= max), the
              roundings add 3 u |d| w + u |mean| <= u (A + 6 D) per merge.  The first merge into an empty accumulator is exact.
              Merges in a chain: L = (prows - 1) + (cpg - 1) + (kmax - 1) + 3 + 7 (`gn_stats_kernel`: lanes, channels of the
              group; `gn_finalize_kernel`: kmax = ceil(nslab / 32) <= 8 slabs per lane, 4 lanes, 8 segments), so
              e_mean = (L + 1) u (A + 6 D) + (g(cnt) + 2 u) 2 D.
              M2 += M2b + d^2 (n nb / tot): exact M2 = sum leaf M2 + sum w2 d^2.  Roundings: 2 u per add and chain level,
              6 u on each w2 d^2 (<= M2 in total).  A mean that is off by e_d = 2 e_mean + 2 u D moves w2 d^2 by
              w2 (2 |d| e_d + e_d^2); sum w2 <= N per level of the hierarchy (5 levels), Cauchy-Schwarz gives
              sum w2 |d| <= sqrt(5 N) sqrt(M2) = sqrt 5 N sigma.  Per sample:
              e_var = (3 g(cnt) + 8 u) 4 D^2 + (2 L + 8) u var + 2 sqrt 5 e_d sigma + 5 e_d^2
              This is what grows with |mean| / spread: e_mean ~ L u A, and the last two terms carry it into rstd.  `Ref.terms`
              holds, per case, |mean| / sigma and the share of each term.
  rstd        r = e_var / (var + eps) + 2 u (division, + eps); rel = r / (2 (1 - r)) + 2 u (v_rsq, assumed) + u (a = rstd gamma)
  element     slack = |x - mu| |a| rel + e_mean |a| + u (|mu a| + |b| + |value|)      (mean * a, beta - ., the fma's rounding)
  SiLU        f * rcp(1 + exp2(-log2e f)): slack' = 1.1 slack + |silu| (|f| + 6) u      (|silu'| <= 1.1; the product inside the
              exponent moves it by u log2e |f|; v_exp 2 u, the add u, v_rcp 2 u, the product u)
GroupNorm from partials (`gn_finalize_cols_kernel`): n = slabs * cpg partials, <= 20 per thread and an 8-level tree: k = 28.
              e_mean = (g(k) + u) max |mean_i|;  e_var = 2 Dp e_mean + e_mean^2 + (g(k) + 5 u) var,  Dp = max |mean_i - mean|.
LayerNorm (`ln_row`): a lane sums cnt = 8 ceil(nchunk / 64) values, the butterfly adds 6 steps: k = cnt + 6.
              e_mean = (g(k) + u) mean |x|;  the second pass is about the computed mean, sum (x - m)^2 = M2 + C e^2 exactly:
              e_var = (g(k) + 4 u) (var + e_mean^2) + e_mean^2;  rstd as above (without the gamma product);
              slack0 = |x - mu| rstd (rel + 2 u) + e_mean rstd;  each of * gamma, + beta, 1 + scale, * (.), + shift adds u of
              its result and scales what came before.
softmax       t = x - max (u |t|), exp(t) = v_exp(t * log2e): u |t| for each of the constant and the product, so
              rel_i = 4 u |t_i| + 2 u;  the sum: 8 ceil(nchunk / 256) (fp32 scores: 4 ceil) per thread + 6 butterfly steps + 3
              adds of the waves: g(k) + the p-weighted mean of rel_j;  1 / sum: 2 u, the product u.
              slack_i = p_i (rel_i + sum_j p_j rel_j + g(k) + 3 u) + 2^-126 (a flushed v_exp result).

`lo` / `hi` are the images of value -+ slack under the output rounding(s) (monotone), not a closed form u |want| + slack: a tie
crossed at the rounding moves a whole ulp.  fp16 results below the smallest normal go through the same image (numpy rounds into
the subnormals as the hardware conversion does).  Nothing here comes from a kernel's output; no term is measured.

Out of scope: offsets beyond 2 GiB; a softmax row that is entirely -inf.  The GroupNorm partials a GEMM / conv writes (`gn_out`),
its LayerNorm partials (`ln_out`) and the LayerNorm fold of the GEMM (`ln_in`) are restated in tests/gemm_fused_ref.py, which hands
the partials of a producing launch to `gnp_reference_of` here.
"""
import collections
import functools
import math

import numpy as np
import torch

from gemm_conv_ref import to_e4m3

U = 2.0 ** -24
SECOND = 1.0 + 2.0 ** -9
F32 = np.float32
GN_MIN_PIX = 8
SENTINEL = 7.0
SENTINEL8 = 0x55
LOG2E32 = F32(1.4426950408889634)

Ref = collections.namedtuple("Ref", "want lo hi bound value slack terms")
Case = collections.namedtuple("Case", "name kind shape dtype opt")


def g_(k):
    return k * U / (1.0 - k * U)


# ---- number formats ---------------------------------------------------------------------------------------------------------------
def rnd(x, dtype):
    """float64 -> the nearest fp16 / bf16 value (ties to even, ONE rounding), as float64."""
    x = np.asarray(x, dtype=np.float64)
    if dtype == "f16":
        with np.errstate(over="ignore"):
            return x.astype(np.float16).astype(np.float64)
    m, e = np.frexp(x)                                # bf16: 8 significant bits; its subnormals (< 2^-126) are not reached here
    out = np.ldexp(np.rint(m * 256.0), e - 8)
    return np.where(np.isfinite(x), out, x)


def rnd32(x, dtype):
    """The kernel's own conversion of an fp32 value."""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=F32))
    return t.to(torch.float16 if dtype == "f16" else torch.bfloat16).double().numpy()


def trunc_bf16(x):
    b = np.ascontiguousarray(x, dtype=F32).view(np.uint32) & np.uint32(0xFFFF0000)
    return b.view(F32).astype(np.float64)


def e4m3(x):
    return to_e4m3(torch.from_numpy(np.ascontiguousarray(x))).numpy()


def tdtype(dtype):
    return torch.float16 if dtype == "f16" else torch.bfloat16


def stored(x32, dtype):
    """(torch tensor of the element type, its values as float64)."""
    t = torch.from_numpy(np.ascontiguousarray(x32, dtype=F32)).to(tdtype(dtype))
    return t, t.double().numpy()


def _rng(name):
    return np.random.default_rng(int.from_bytes(name.encode(), "little") % (2 ** 63))


# ---- GroupNorm: the host formulas of iir_groupnorm_nhwc ---------------------------------------------------------------------
Geo = collections.namedtuple("Geo", "nslab0 nslab pps last nchunk lanes_c prows idle passes loop4 cpg gblocks kmax nblk ppb cnt")


def gn_geo(R, HW, C, G):
    nslab = (HW + GN_MIN_PIX - 1) // GN_MIN_PIX
    nslab = max(1, min(nslab, (1024 + R - 1) // R, 256))
    nslab0 = nslab
    pps = (HW + nslab - 1) // nslab
    nslab = (HW + pps - 1) // pps
    last = HW - (nslab - 1) * pps
    nchunk = C // 8
    lanes_c = min(nchunk, 256)
    prows = 256 // lanes_c
    loop4 = set()                       # how often the 4-deep loop runs, over every (slab length, lane)
    cnt = 1
    for n in {pps, last}:
        for tp in range(prows):
            p, k = tp, 0
            while p + 3 * prows < n:
                p += 4 * prows
                k += 1
            loop4.add(k)
            cnt = max(cnt, (n - tp + prows - 1) // prows if tp < n else 0)
    nblk = (1024 + R - 1) // R
    ppb = max((HW + nblk - 1) // nblk, GN_MIN_PIX)
    nblk = (HW + ppb - 1) // ppb
    return Geo(nslab0, nslab, pps, last, nchunk, lanes_c, prows, 256 % lanes_c != 0, (nchunk + lanes_c - 1) // lanes_c, loop4, C // G,
               (G + 7) // 8, (nslab + 31) // 32, nblk, ppb, cnt)


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=8)
def gn_input(shape, dtype, mode):
    """x (R, HW, C) as stored values (float64) and as a tensor: noise, a ramp along the pixels, an offset per slab, per channel and
    per image, a step on the last slab (every tail position differs from the body), then the mode: "c" centred, "lm300" / "lm1000"
    a mean of 300 / 1000 spreads, "tiny" a variance near eps."""
    R, HW, C, G = shape
    geo = gn_geo(R, HW, C, G)
    rng = _rng(f"gn{shape}")
    p = np.arange(HW)
    x = rng.standard_normal((R, HW, C)) * 0.5
    x += (1.5 * (p / HW - 0.5) + 0.3 * ((p // geo.pps) % 5 - 2) + 1.0 * (p >= (geo.nslab - 1) * geo.pps) + 0.01 * (p % 13))[None, :, None]
    x += (0.4 * ((np.arange(C) % 7) - 3) / 3)[None, None, :]
    x += (0.3 * (np.arange(R) % 3))[:, None, None]
    if mode.startswith("lm"):
        x += float(mode[2:]) * 0.9
    elif mode == "tiny":
        x *= 3e-3
    t, v = stored(x.astype(F32), dtype)
    rg = _rng(f"gnaff{shape}")
    gm, _ = stored((1.0 + 0.5 * rg.standard_normal(C)).astype(F32), dtype)
    bt, _ = stored((0.5 * rg.standard_normal(C)).astype(F32), dtype)
    return t.reshape(R * HW, C), v, gm, bt


@functools.lru_cache(maxsize=8)
def gn_partials(shape, dtype, mode):
    """fp32 (R * HW / 64, C, 2): (mean, M2) of every 64-row slab and channel, in fp64 from the stored x, rounded to fp32."""
    R, HW, C, G = shape
    v = gn_input(shape, dtype, mode)[1].reshape(R * HW // 64, 64, C)
    m = v.mean(1)
    return np.stack([m, ((v - m[:, None]) ** 2).sum(1)], -1).astype(F32)


# ---- GroupNorm: the reference -----------------------------------------------------------------------------------------------
def silu64(f):
    with np.errstate(over="ignore"):
        return f / (1.0 + np.exp(-f))


def gnp_stats64(part, R, G):
    """The `partials=` form on ANY fp32 partials (R * HW / 64, C, 2): per (image, group) mean, var and the error of the kernel's."""
    slabs, C = part.shape[0] // R, part.shape[1]
    cpg = C // G
    pt = np.asarray(part).astype(np.float64).reshape(R, slabs, G, cpg, 2)
    pm = pt[..., 0].transpose(0, 2, 1, 3).reshape(R, G, -1)
    mean = pm.mean(-1)
    dp = np.abs(pm - mean[..., None])
    var = (pt[..., 1].transpose(0, 2, 1, 3).reshape(R, G, -1).sum(-1) + 64.0 * (dp ** 2).sum(-1)) / (pm.shape[-1] * 64.0)
    k = 28
    e_mean = (g_(k) + U) * np.abs(pm).max(-1)
    e_var = 2 * dp.max(-1) * e_mean + e_mean ** 2 + (g_(k) + 5 * U) * var
    return mean, var, e_mean, e_var, dict(chain=k)


@functools.lru_cache(maxsize=8)
def _gn_stats64(shape, dtype, mode, partials):
    """Per (image, group): mean, var, and the error of the kernel's mean / var (see the module docstring) with its terms."""
    R, HW, C, G = shape
    geo = gn_geo(R, HW, C, G)
    cpg = C // G
    if partials:
        return gnp_stats64(gn_partials(shape, dtype, mode), R, G)
    else:
        v = gn_input(shape, dtype, mode)[1].reshape(R, HW, G, cpg)
        mean = v.mean((1, 3))
        var = v.var((1, 3))
        A = np.abs(v).max((1, 3))
        D = np.abs(v - mean[:, None, :, None]).max((1, 3))
        sig = np.sqrt(var)
        L = (geo.prows - 1) + (cpg - 1) + (geo.kmax - 1) + 3 + 7
        e_mean = (L + 1) * U * (A + 6 * D) + (g_(geo.cnt) + 2 * U) * 2 * D
        e_d = 2 * e_mean + 2 * U * D
        t_thread, t_round, t_cross = (3 * g_(geo.cnt) + 8 * U) * 4 * D ** 2, (2 * L + 8) * U * var, 2 * math.sqrt(5) * e_d * sig + 5 * e_d ** 2
        e_var = t_thread + t_round + t_cross
        with np.errstate(divide="ignore", invalid="ignore"):
            terms = dict(chain=L, mean_over_sigma=float(np.nanmax(np.where(sig > 0, np.abs(mean) / sig, 0))),
                         e_mean_over_sigma=float(np.nanmax(np.where(sig > 0, e_mean / sig, 0))),
                         var_thread=float((t_thread / (var + 1e-30)).max()), var_round=float((t_round / (var + 1e-30)).max()),
                         var_cross=float((t_cross / (var + 1e-30)).max()))
    return mean, var, e_mean, e_var, terms


def gn_reference(cs, rounding=True):
    R, HW, C, G = cs.shape
    o = cs.opt
    mode, eps, silu, partials = o["mode"], o["eps"], o["silu"], cs.kind == "gnp"
    _, v, gm, bt = gn_input(cs.shape, cs.dtype, mode)
    stats = _gn_stats64(cs.shape, cs.dtype, mode, partials)
    return _gn_apply(cs.name, cs.shape, cs.dtype, v, gm.double().numpy(), bt.double().numpy(), stats, eps, silu, rounding)


def gnp_reference_of(name, shape, dtype, v, gm, bt, part, eps, silu):
    """`gn_reference` of the `partials=` form for operands that do not come from `gn_input`: v (R, HW, C) the stored x as float64,
    gm / bt float64 (C,), part the fp32 partials a producing launch left (tests/test_gemm_fused_every_build_gpu.py)."""
    return _gn_apply(name, shape, dtype, v, gm, bt, gnp_stats64(part, shape[0], shape[3]), eps, silu, True)


def _gn_apply(name, shape, dtype, v, gm, bt, stats, eps, silu, rounding):
    R, HW, C, G = shape
    mean, var, e_mean, e_var, terms = stats
    cpg = C // G
    rstd = 1.0 / np.sqrt(var + eps)
    r = e_var / (var + eps) + 2 * U
    assert r.max() < 2.0 ** -5, (name, r.max())
    rel = r / (2 * (1 - r)) + 3 * U
    ex = lambda t: np.repeat(t, cpg, axis=1)[:, None, :]           # (R, G) -> (R, 1, C)
    a = ex(rstd) * gm
    b = bt - ex(mean) * a
    value = v * a + b
    slack = (np.abs(v - ex(mean)) * np.abs(a) * ex(rel) + ex(e_mean) * np.abs(a) + U * (np.abs(ex(mean) * a) + np.abs(b) + np.abs(value)))
    if silu:
        f = value
        value = silu64(f)
        slack = 1.1 * slack + np.abs(value) * (np.abs(f) + 6) * U + 2.0 ** -126
    slack = slack * SECOND
    value, slack = value.reshape(R * HW, C), slack.reshape(R * HW, C)
    if not rounding:
        return value
    terms = dict(terms, rstd_rel=float(rel.max()))
    return _finish(value, slack, dtype, terms)


def _finish(value, slack, dtype, terms, fp8=False):
    want, lo, hi = rnd(value, dtype), rnd(value - slack, dtype), rnd(value + slack, dtype)
    if fp8:
        want, lo, hi = e4m3(want), e4m3(lo), e4m3(hi)
    return Ref(want, lo, hi, np.maximum(hi - want, want - lo), value, slack, terms)


# ---- GroupNorm: the stand-in ------------------------------------------------------------------------------------------------
def fma(a, b, c, fused):
    if fused:
        return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)
    return (a * b).astype(F32) + c


def chan_merge(n, mean, m2, nb, mb, m2b, fused):
    """`chan_merge` of csrc/norm.hip on fp32 arrays (nb <= 0: unchanged)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        n, mean, m2, nb, mb, m2b = np.broadcast_arrays(*(np.asarray(t, F32) for t in (n, mean, m2, nb, mb, m2b)))
        tot = n + nb
        d = mb - mean
        mean2 = fma(d, nb / tot, mean, fused)
        m22 = m2 + fma(d * d, (n * nb) / tot, m2b, fused)
    on = nb > 0
    return np.where(on, tot, n), np.where(on, mean2, mean), np.where(on, m22, m2)


def rsq32(x):
    with np.errstate(divide="ignore", invalid="ignore"):
        return (1.0 / np.sqrt(np.asarray(x, np.float64))).astype(F32)


def _gn_stats_standin(x, geo, G, fused, mut):
    """`gn_stats_kernel`: (mean, M2) per (image, slab, group), fp32."""
    R, HW, C = x.shape
    pps, nslab, prows, cpg = geo.pps, geo.nslab, geo.prows, geo.cpg
    iters = (pps + prows - 1) // prows
    off = np.arange(iters)[:, None] * prows + np.arange(prows)[None, :]                  # (iters, prows): pixel within the slab
    p0 = np.arange(nslab) * pps
    p1 = np.minimum(HW, p0 + pps)
    pix = p0[:, None, None] + off[None]
    valid = pix < p1[:, None, None]
    first_ok = valid[:, 0]
    if mut == "tail_dropped":
        valid = valid & (pix != (p1 - 1)[:, None, None])
    xg = x[:, np.minimum(pix, HW - 1)]                                                 # (R, nslab, iters, prows, C)
    k0 = np.where(first_ok[None, :, :, None], xg[:, :, 0], F32(0))
    s = np.zeros_like(k0)
    q = np.zeros_like(k0)
    cnt = np.zeros(valid[:, 0].shape, F32)
    for i in range(iters):
        ok = valid[None, :, i, :, None]
        f = xg[:, :, i] - k0
        s = np.where(ok, s + f, s)
        q = np.where(ok, fma(f, f, q, fused), q)
        cnt = cnt + valid[:, i]
    with np.errstate(divide="ignore"):
        inv = np.where(cnt > 0, F32(1) / cnt, F32(0)).astype(F32)[None, :, :, None]
    cmean = fma(s, inv, k0, fused)
    cm2 = np.maximum(fma(-(s * s), inv, q, fused), F32(0))
    nt = np.where(p0[:, None] + np.arange(prows)[None] < p1[:, None], (p1[:, None] - p0[:, None] - np.arange(prows)[None] + prows - 1) // prows, 0)
    nt = nt.astype(F32)
    if mut == "nt_off_by_one" and prows > 1:
        nt[:, prows - 1] += 1
    n = np.zeros((1, nslab, 1), F32)
    mean = np.zeros((R, nslab, C), F32)
    m2 = np.zeros((R, nslab, C), F32)
    for t in range(prows):
        n, mean, m2 = chan_merge(n, mean, m2, nt[None, :, t, None], cmean[:, :, t], cm2[:, :, t], fused)
    npix = (p1 - p0).astype(F32)[None, :, None]
    chm, chq = mean.reshape(R, nslab, G, cpg), m2.reshape(R, nslab, G, cpg)
    n = np.zeros((1, nslab, 1), F32)
    gm, gq = np.zeros((R, nslab, G), F32), np.zeros((R, nslab, G), F32)
    for c in range(cpg):
        n, gm, gq = chan_merge(n, gm, gq, npix, chm[..., c], chq[..., c], fused)
    return gm, gq


def _gn_finalize_standin(pm, pq, geo, HW, eps, fused, mut):
    """`gn_finalize_kernel` on partials (R, nslab, G): (mean, rstd) per (image, group)."""
    R, nslab, G = pm.shape
    pps, cpg = geo.pps, geo.cpg
    nloop = nslab
    if mut == "stale_workspace" and geo.nslab0 > nslab:
        nloop = geo.nslab0
        pad = np.full((R, nloop - nslab, G), np.nan, F32)
        pm, pq = np.concatenate([pm, pad], 1), np.concatenate([pq, pad], 1)
    p0 = np.arange(nloop) * pps
    cnts = (np.minimum(HW, p0 + pps) - p0) * cpg
    if mut == "last_slab_full":
        cnts = np.full(nloop, pps * cpg)
    if mut == "stale_workspace":
        cnts = np.where(cnts > 0, cnts, pps * cpg)
    cnts = cnts.astype(F32)
    n, mean, m2 = np.zeros((1, 32, 1), F32), np.zeros((R, 32, G), F32), np.zeros((R, 32, G), F32)
    for k in range(1 if mut == "slabs_beyond_32" else 8):
        sidx = np.arange(32) + 32 * k
        ok = sidx < nloop
        sc = np.minimum(sidx, nloop - 1)
        n, mean, m2 = chan_merge(n, mean, m2, np.where(ok, cnts[sc], 0)[None, :, None], pm[:, sc], pq[:, sc], fused)
    n = np.broadcast_to(n, mean.shape)
    tn, tm, tq = np.zeros((R, 8, G), F32), np.zeros((R, 8, G), F32), np.zeros((R, 8, G), F32)
    for l in range(4):
        src = np.arange(8) * 4 + l
        tn, tm, tq = chan_merge(tn, tm, tq, n[:, src], mean[:, src], m2[:, src], fused)
    fn, fm, fq = np.zeros((R, G), F32), np.zeros((R, G), F32), np.zeros((R, G), F32)
    for sg in range(8):
        fn, fm, fq = chan_merge(fn, fm, fq, tn[:, sg], tm[:, sg], tq[:, sg], fused)
    with np.errstate(divide="ignore", invalid="ignore"):
        if mut == "var_nm1":
            var = fq / (fn - F32(1))
        else:
            var = fq / fn
        if mut == "eps_after_sqrt":
            rstd = (F32(1) / (np.sqrt(var).astype(F32) + F32(eps))).astype(F32)
        else:
            rstd = rsq32(var + F32(eps))
    return fm, rstd


def _gn_cols_standin(part, R, G, cpg, eps, slab_len):
    """`gn_finalize_cols_kernel`: partials (R * slabs, C, 2) fp32 -> (mean, rstd) per (image, group)."""
    slabs = part.shape[0] // R
    n = slabs * cpg
    a = part.reshape(R, slabs, G, cpg, 2).transpose(0, 2, 1, 3, 4).reshape(R, G, n, 2)
    pad = np.zeros((R, G, 20 * 256 - n, 2), F32)
    a = np.concatenate([a, pad], 2).reshape(R, G, 20, 256, 2)
    ok = (np.arange(20)[:, None] * 256 + np.arange(256)[None, :]) < n

    def block_sum(v):
        red = v.copy()
        o = 128
        while o > 0:
            red[..., :o] = red[..., :o] + red[..., o:2 * o]
            o >>= 1
        return red[..., 0]
    sm = np.zeros((R, G, 256), F32)
    for k in range(20):
        sm = sm + np.where(ok[k], a[:, :, k, :, 0], F32(0))
    mean = block_sum(sm) / F32(n)
    q = np.zeros((R, G, 256), F32)
    for k in range(20):
        d = a[:, :, k, :, 0] - mean[..., None]
        q = q + np.where(ok[k], fma(F32(slab_len) * d, d, a[:, :, k, :, 1], True), F32(0))
    m2 = block_sum(q)
    return mean, rsq32(m2 / (F32(n) * F32(slab_len)) + F32(eps))


def silu32(f):
    """`silu_f`: x * rcp(1 + exp2(-log2e * x)) with each fp32 operation rounded once."""
    with np.errstate(over="ignore", divide="ignore"):
        e = np.exp2((-LOG2E32 * f).astype(np.float64)).astype(F32)
        return f * (1.0 / (F32(1) + e).astype(np.float64)).astype(F32)


def out_geometry(cs):
    """(buffer rows, ld, first row, first column) of the output buffer the GPU file makes for `cs`; `x_geometry` likewise."""
    rows, C = out_shape(cs)
    return rows + 3, C + 40, 1, 16


def x_geometry(cs):
    rows, C = in_shape(cs)
    return rows + 2, C + 24, 1, 8


def in_shape(cs):
    if cs.kind in ("gn", "gnp"):
        R, HW, C, G = cs.shape
        return R * HW, C
    return cs.shape


def out_shape(cs):
    if cs.kind == "ln" and cs.opt.get("tr"):
        rows, C = cs.shape
        return C, tr_col(rows - 1, cs.opt) + 1
    return in_shape(cs)


def tr_col(row, o):
    return (row // o["tr_rows"]) * o["tr_bstride"] + row % o["tr_rows"]


def _wrong_stride(cs, res, fill):
    """The mutant that stores row i at i * ldx: what the output VIEW then holds (rows that land outside the buffer are lost)."""
    nb, ld, r0, c0 = out_geometry(cs)
    ldx = x_geometry(cs)[1]
    flat = np.full(nb * ld + res.shape[1], fill, np.float64)
    base = r0 * ld + c0
    for i in range(res.shape[0]):
        at = base + i * ldx
        if at + res.shape[1] <= nb * ld:
            flat[at:at + res.shape[1]] = res[i]
    return flat[:nb * ld].reshape(nb, ld)[r0:r0 + res.shape[0], c0:c0 + res.shape[1]].copy()


@functools.lru_cache(maxsize=4)
def _gn_standin_stats(shape, dtype, mode, partials, eps, fused, mut):
    R, HW, C, G = shape
    geo = gn_geo(R, HW, C, G)
    v = gn_input(shape, dtype, mode)[1]
    if partials:
        return _gn_cols_standin(gn_partials(shape, dtype, mode), R, G, geo.cpg, eps, geo.pps if mut == "cols_true_slab_len" else 64)
    x = v.astype(F32)
    if mut == "var_ex2":
        xg = x.reshape(R, HW, G, geo.cpg)
        N = F32(HW * geo.cpg)
        mean = xg.sum((1, 3), dtype=F32) / N
        var = (xg * xg).sum((1, 3), dtype=F32) / N - mean * mean
        return mean, rsq32(np.maximum(var, F32(0)) + F32(eps))
    pm, pq = _gn_stats_standin(x, geo, G, fused, mut)
    mean, rstd = _gn_finalize_standin(pm, pq, geo, HW, eps, fused, mut)
    if mut == "gi_mask_dropped" and G % 8 and R > 1:
        # lanes gi in [G, 8 * gblocks) read one slab further on and write the NEXT image's (mean, rstd) of group gi - G
        ng = min(geo.gblocks * 8 - G, G)
        fm = pm.reshape(R * geo.nslab, G)[1:1 + (R - 1) * geo.nslab].reshape(R - 1, geo.nslab, G)[..., :ng]
        fq = pq.reshape(R * geo.nslab, G)[1:1 + (R - 1) * geo.nslab].reshape(R - 1, geo.nslab, G)[..., :ng]
        m_, r_ = _gn_finalize_standin(fm, fq, geo, HW, eps, fused, None)
        mean, rstd = mean.copy(), rstd.copy()
        mean[1:, :ng], rstd[1:, :ng] = m_, r_
    return mean, rstd


GN_MUTANTS = ("var_ex2", "var_nm1", "eps_after_sqrt", "last_slab_full", "tail_dropped", "nt_off_by_one", "slabs_beyond_32",
              "group_from_chunk", "gi_mask_dropped", "silu_before_affine", "ldx_for_ldy", "stale_workspace", "cols_true_slab_len")
_GN_STAT_MUTANTS = ("var_ex2", "var_nm1", "eps_after_sqrt", "last_slab_full", "tail_dropped", "nt_off_by_one", "slabs_beyond_32",
                    "gi_mask_dropped", "stale_workspace", "cols_true_slab_len")


def gn_standin(cs, fused=True, mut=None):
    R, HW, C, G = cs.shape
    o = cs.opt
    _, v, gm, bt = gn_input(cs.shape, cs.dtype, o["mode"])
    mean, rstd = _gn_standin_stats(cs.shape, cs.dtype, o["mode"], cs.kind == "gnp", o["eps"], fused, mut if mut in _GN_STAT_MUTANTS else None)
    cpg = C // G
    ch = np.arange(C)
    gi = (ch // 8 * 8) // cpg if mut == "group_from_chunk" else ch // cpg
    x = v.astype(F32)
    gm32, bt32 = gm.float().numpy(), bt.float().numpy()
    rs, mn = rstd[:, gi][:, None, :], mean[:, gi][:, None, :]
    if mut == "silu_before_affine" and o["silu"]:
        f = fma(silu32(fma(x, rs, -(mn * rs), True)), gm32, bt32, True)
    else:
        a = rs * gm32
        b = fma(-mn, a, bt32, fused)
        f = fma(x, a, b, True)                       # an explicit fmaf in gn_apply_kernel
        if o["silu"]:
            f = silu32(f)
    res = rnd32(f, cs.dtype).reshape(R * HW, C)
    if mut == "ldx_for_ldy":
        res = _wrong_stride(cs, res, SENTINEL)
    return res


# ---- LayerNorm ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ln_input(shape):
    """x (rows, C) fp16: rows of different mean and spread (every fourth one with a mean of 300 spreads, every eighth one with a
    variance near eps); gamma, beta; shift and
    scale with one distinct row per `rows_per_mod` rows (16 rows at least, so a wrong row index has somewhere to land)."""
    rows, C = shape
    rng = _rng(f"ln{shape}")
    x = rng.standard_normal((rows, C)) * (0.5 + (np.arange(rows) % 3))[:, None] + (np.arange(rows) % 5 - 2)[:, None] * 0.7
    x += 0.2 * (np.arange(C) % 11)[None, :]
    x[3::4] = x[3::4] * 0.25 + 75.0
    x[2::8] *= 2e-3                                   # a variance of the size of eps
    xt, xv = stored(x.astype(F32), "f16")
    gm = stored((1.0 + 0.5 * rng.standard_normal(C)).astype(F32), "f16")
    bt = stored((0.5 * rng.standard_normal(C)).astype(F32), "f16")
    nmod = 16
    sh = stored((0.5 * rng.standard_normal((nmod, C)) + 0.1 * np.arange(nmod)[:, None]).astype(F32), "f16")
    sc = stored((0.3 * rng.standard_normal((nmod, C)) - 0.05 * np.arange(nmod)[:, None]).astype(F32), "f16")
    return xt, xv, gm, bt, sh, sc


def ln_reference(cs, rounding=True):
    rows, C = cs.shape
    o = cs.opt
    _, x, gm, bt, sh, sc = ln_input(cs.shape)
    eps = o["eps"]
    mean = x.mean(1, keepdims=True)
    var = x.var(1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + eps)
    nchunk = C // 8
    k = 8 * ((nchunk + 63) // 64) + 6
    e_mean = (g_(k) + U) * np.abs(x).mean(1, keepdims=True)
    e_var = (g_(k) + 4 * U) * (var + e_mean ** 2) + e_mean ** 2
    r = e_var / (var + eps) + 2 * U
    rel = r / (2 * (1 - r)) + 2 * U
    assert rel.max() < 2.0 ** -9, (cs.name, rel.max())
    value = (x - mean) * rstd
    slack = np.abs(value) * (rel + 2 * U) + e_mean * rstd
    if "g" in o["affine"]:
        value = value * gm[1]
        slack = slack * np.abs(gm[1]) + U * np.abs(value)
    if "b" in o["affine"]:
        value = value + bt[1]
        slack = slack + U * np.abs(value)
    if o.get("ada"):
        mrow = np.arange(rows) // o["rpm"]
        one = 1.0 + sc[1][mrow]
        prod = value * one
        value = prod + sh[1][mrow]
        slack = slack * np.abs(one) + 2 * U * np.abs(prod) + U * np.abs(value)
    slack = slack * SECOND
    if o.get("tr"):
        value, slack = _transpose(value, o, 0.0), _transpose(slack, o, 0.0)
    if not rounding:
        return value
    terms = dict(chain=k, mean_over_sigma=float((np.abs(mean) / np.sqrt(var)).max()), rstd_rel=float(rel.max()))
    return _finish(value, slack, "f16", terms, fp8=bool(o.get("fp8")))


def _transpose(val, o, fill, col=None):
    rows, C = val.shape
    cols = [tr_col(r, o) if col is None else col(r) for r in range(rows)]
    out = np.full((C, tr_col(rows - 1, o) + 1), fill, np.float64)
    out[:, cols] = val.T
    return out


def written_mask(cs):
    """True where the launch writes the output view (the transposed form leaves the columns between the batches alone)."""
    if cs.kind == "ln" and cs.opt.get("tr"):
        return _transpose(np.ones(cs.shape), cs.opt, 0.0) > 0
    return np.ones(out_shape(cs), bool)


def wave_sum32(v):
    """`wave_sum`: the 6-step xor butterfly over the last axis (64 lanes); every lane ends with the same value."""
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ o]
    return v[..., 0]


LN_MUTANTS = ("ln_mean_full_pass", "ln_scale_no_one", "ln_shift_scale_swapped", "ln_mod_row_modulo", "ln_tr_no_bstride", "ln_fp8_from_fp32",
              "ln_eps_after_sqrt")


def ln_standin(cs, fused=True, mut=None):
    rows, C = cs.shape
    o = cs.opt
    _, xv, gm, bt, sh, sc = ln_input(cs.shape)
    nchunk = C // 8
    K = 5
    ch = np.arange(64)[None, :] + 64 * np.arange(K)[:, None]                         # (K, 64)
    ok = ch < nchunk
    v = xv.astype(F32).reshape(rows, nchunk, 8)[:, np.minimum(ch, nchunk - 1)]            # (rows, K, 64, 8)
    s = np.zeros((rows, 64), F32)
    for k in range(K):
        for j in range(8):
            s = np.where(ok[k], s + v[:, k, :, j], s)
    div = F32(((nchunk + 63) // 64) * 64 * 8 if mut == "ln_mean_full_pass" else C)
    mean = (wave_sum32(s) / div)[:, None]
    q = np.zeros((rows, 64), F32)
    for k in range(K):
        for j in range(8):
            d = v[:, k, :, j] - mean
            q = np.where(ok[k], fma(d, d, q, fused), q)
    var = wave_sum32(q) / F32(C)
    if mut == "ln_eps_after_sqrt":
        rstd = (F32(1) / (np.sqrt(var).astype(F32) + F32(o["eps"]))).astype(F32)[:, None]
    else:
        rstd = rsq32(var + F32(o["eps"]))[:, None]
    x = xv.astype(F32)
    f = (x - mean) * rstd
    g32, b32 = gm[0].float().numpy(), bt[0].float().numpy()
    if "g" in o["affine"] and "b" in o["affine"]:
        f = fma(f, g32, b32, fused)
    elif "g" in o["affine"]:
        f = f * g32
    elif "b" in o["affine"]:
        f = f + b32
    if o.get("ada"):
        r = np.arange(rows)
        mrow = np.minimum(r % o["rpm"] if mut == "ln_mod_row_modulo" else r // o["rpm"], sh[1].shape[0] - 1)
        s32, c32 = sh[0].float().numpy()[mrow], sc[0].float().numpy()[mrow]
        if mut == "ln_shift_scale_swapped":
            s32, c32 = c32, s32
        f = fma(f, c32 if mut == "ln_scale_no_one" else F32(1) + c32, s32, fused)
    res = rnd32(f, "f16")
    if o.get("fp8"):
        res = e4m3(f.astype(np.float64) if mut == "ln_fp8_from_fp32" else res)
    if o.get("tr"):
        res = _transpose(res, o, SENTINEL, (lambda r: r) if mut == "ln_tr_no_bstride" else None)
    return res


# ---- softmax ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sm_input(kind, shape):
    """rows x cols scores (fp16 or fp32): row 0 one dominant element (in the last chunk: another wave than lane 0's unless the row
    is one chunk); row 1 all elements equal; row 2 scores around 1000 (fp32: 10^4) with a spread of 6, far outside the range of exp
    in either format, with -inf, -3e4 (fp32: -1e30) and -300 entries beside them."""
    rows, cols = shape
    rng = _rng(f"sm{shape}{kind}")
    x = rng.standard_normal((rows, cols)) * 2.0
    x[0, cols - 3] = 40.0
    x[1] = -3.25
    big, off = (3.0e4, 1000.0) if kind == "sm16" else (1.0e30, 1.0e4)
    x[2] = off + rng.standard_normal(cols) * 6.0
    x[2, ::7] = -np.inf
    x[2, 1::11] = -big
    x[2, 2::13] = off - 300.0
    x[2, cols // 2 + 1] = off + 12.0
    if kind == "sm16":
        return stored(x.astype(F32), "f16")
    t = torch.from_numpy(x.astype(F32))
    return t, t.double().numpy()


def sm_reference(cs, rounding=True):
    rows, cols = cs.shape
    x = sm_input(cs.kind, cs.shape)[1]
    with np.errstate(invalid="ignore"):
        t = x - x.max(1, keepdims=True)
    e = np.exp(t)
    p = e / e.sum(1, keepdims=True)
    if not rounding:
        return p
    per = 8 if cs.kind == "sm16" else 4
    k = per * ((cols // per + 255) // 256) + 6 + 3
    at = np.where(np.isfinite(t), np.abs(t), 0.0)
    rel = 4 * U * at + 2 * U
    slack = (p * (rel + (p * rel).sum(1, keepdims=True) + g_(k) + 3 * U) + 2.0 ** -126) * SECOND
    slack = np.where(p > 0, slack, np.where(np.isfinite(t), 2.0 ** -126, 0.0))
    return _finish(p, slack, cs.dtype, dict(chain=k))


SM_MUTANTS = ("sm_max_one_wave", "sm_sum_one_wave", "sm_clamped_dup", "sm_bf16_trunc")


def sm_standin(cs, fused=True, mut=None):
    rows, cols = cs.shape
    x = sm_input(cs.kind, cs.shape)[1].astype(F32)
    per, K = (8, 8) if cs.kind == "sm16" else (4, 16)
    nchunk = cols // per
    ch = np.arange(256)[None, :] + 256 * np.arange(K)[:, None]                       # (K, 256)
    ok = ch < nchunk
    v = x.reshape(rows, nchunk, per)[:, np.minimum(ch, nchunk - 1)]                       # (rows, K, 256, per)
    tmax = np.where(ok[None, :, :, None], v, F32(-np.inf)).max((1, 3))                   # per thread
    wmax = tmax.reshape(rows, 4, 64).max(2)
    if mut == "sm_max_one_wave":
        mx = np.repeat(wmax, 64, axis=1)[:, None, :, None]                               # every wave keeps its own maximum
    else:
        mx = wmax.max(1)[:, None, None, None]
    with np.errstate(invalid="ignore", over="ignore"):
        t = (v - mx).astype(F32)
        e = np.exp2((t * LOG2E32).astype(np.float64)).astype(F32)
    s = np.zeros((rows, 256), F32)
    for k in range(K):
        for j in range(per):
            s = np.where(ok[k] | (mut == "sm_clamped_dup"), s + e[:, k, :, j], s)
    ws = np.stack([wave_sum32(s[:, w * 64:(w + 1) * 64]) for w in range(4)], 1)
    tot = ws[:, 0] if mut == "sm_sum_one_wave" else ((ws[:, 0] + ws[:, 1]) + ws[:, 2]) + ws[:, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = (F32(1) / tot)[:, None, None, None]
        o = (e * inv).astype(F32)
    out = np.zeros((rows, nchunk, per), F32)
    out[:, ch[ok]] = o[:, ok]
    out = out.reshape(rows, cols)
    if mut == "sm_bf16_trunc" and cs.dtype == "bf16":
        return trunc_bf16(out)
    return rnd32(out, cs.dtype)


# ---- the table ----------------------------------------------------------------------------------------------------------------
MUTANTS = GN_MUTANTS + LN_MUTANTS + SM_MUTANTS

GN_SHAPES = ((1, 1, 64, 32), (1, 7, 64, 64), (3, 100, 960, 32), (64, 256, 64, 4), (64, 250, 320, 32), (2, 2600, 320, 32),
             (1, 4100, 72, 12),          # 12 groups need C % 12 == 0: 72 channels, 6 per group (a group boundary inside a chunk)
             (1, 64, 2560, 32), (2, 328, 2560, 32))
GN_EXTRA = ((1, 2041, 64, 32),           # 256 slabs, the last one a single pixel
            (1, 4100, 960, 32))          # prows = 2, 17-pixel slabs: the 4-deep loop twice and a tail after it
GNP_SHAPES = ((1, 64, 64, 64), (2, 64 * 257, 64, 64), (2, 32768, 80, 8), (2, 1024, 320, 32))
LN_CS = (8, 64, 504, 512, 520, 1280, 2048, 2552, 2560)
LN_ROWS = (1, 5, 37)
SM16_COLS = (8, 2040, 2048, 2056, 16376, 16384)
SM32_COLS = (4, 4092, 4096, 4100, 16380, 16384)


def _cases():
    out = []

    def add(name, kind, shape, dtype, **opt):
        out.append(Case(name, kind, tuple(shape), dtype, opt))

    def gn_name(kind, shape, dt, silu, eps, mode):
        R, HW, C, G = shape
        return f"{kind}.{R}x{HW}x{C}g{G}.{dt}.{'silu' if silu else 'lin'}.e{5 if eps == 1e-5 else 6}" + ("" if mode == "c" else "." + mode)

    def gn(kind, shape, dt, silu, eps, mode="c"):
        add(gn_name(kind, shape, dt, silu, eps, mode), kind, shape, dt, silu=silu, eps=eps, mode=mode)

    for shape in GN_SHAPES:
        for dt in ("f16", "bf16"):
            for silu in (True, False):
                for eps in (1e-5, 1e-6):
                    gn("gn", shape, dt, silu, eps)
    for shape in GN_EXTRA:
        gn("gn", shape, "f16", True, 1e-5)
        gn("gn", shape, "bf16", False, 1e-6)
    gn("gn", (2, 2600, 320, 32), "f16", True, 1e-5, "lm300")
    gn("gn", (2, 2600, 320, 32), "bf16", False, 1e-6, "lm300")
    gn("gn", (2, 2600, 320, 32), "f16", False, 1e-6, "lm1000")
    gn("gn", (1, 4100, 72, 12), "f16", True, 1e-6, "lm300")
    gn("gn", (3, 100, 960, 32), "f16", False, 1e-5, "lm300")
    gn("gn", (3, 100, 960, 32), "f16", False, 1e-5, "tiny")
    gn("gn", (3, 100, 960, 32), "bf16", True, 1e-6, "tiny")
    for shape in GNP_SHAPES:
        gn("gnp", shape, "f16", True, 1e-5)
        gn("gnp", shape, "bf16", False, 1e-6)
    gn("gnp", (2, 1024, 320, 32), "f16", False, 1e-6, "lm300")
    for C in LN_CS:
        for rows in LN_ROWS:
            for aff in ("gb", "g", "b", ""):
                add(f"ln.c{C}.r{rows}.{aff or 'none'}", "ln", (rows, C), "f16", affine=aff, eps=1e-5)
        add(f"ln.ada.c{C}", "ln", (37, C), "f16", affine="", eps=1e-6, ada=True, rpm=16)
        add(f"ln.tr.c{C}", "ln", (37, C), "f16", affine="", eps=1e-6, ada=True, rpm=16, tr=True, tr_rows=16, tr_bstride=24)
        add(f"ln.fp8.c{C}", "ln", (37, C), "f16", affine="gb", eps=1e-5, fp8=True)
    for cols in SM16_COLS:
        add(f"sm16.c{cols}", "sm16", (3, cols), "f16")
    for cols in SM32_COLS:
        for dt in ("f16", "bf16"):
            add(f"sm32.c{cols}.{dt}", "sm32", (3, cols), dt)
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return {c.name: c for c in out}


CASES = _cases()
ADALN_JOBS = tuple((C, tr) for C in (8, 320, 2560) for tr in (False, True))          # rows = 37 (% 4 != 0), rows_per_mod = 16


def adaln_case(C, tr):
    o = dict(affine="", eps=1e-6, ada=True, rpm=16)
    if tr:
        o.update(tr=True, tr_rows=16, tr_bstride=24)
    return Case(f"adaln.c{C}.{'tr' if tr else 'n'}", "ln", (37, C), "f16", o)


def reference(cs, rounding=True):
    return {"gn": gn_reference, "gnp": gn_reference, "ln": ln_reference, "sm16": sm_reference, "sm32": sm_reference}[cs.kind](cs, rounding)


def standin(cs, fused=True, mut=None):
    return {"gn": gn_standin, "gnp": gn_standin, "ln": ln_standin, "sm16": sm_standin, "sm32": sm_standin}[cs.kind](cs, fused, mut)


def compare(got, ref, mask=None):
    """(elements outside [lo, hi] or not finite, the worst |got - want| / bound: inf where the bound is 0 and the error is not)."""
    got = np.asarray(got, np.float64)
    err = np.abs(got - ref.want)
    err = np.where(np.isfinite(got), err, np.inf)
    bad = err > ref.bound
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err > 0, err / ref.bound, 0.0)
    if mask is not None:
        bad, ratio = bad & mask, np.where(mask, ratio, 0.0)
    return int(bad.sum()), float(ratio.max())


def ulp_of(want, cs):
    """The spacing of the output format at `want` (the last of the two formats for an fp8 out)."""
    a = np.abs(want)
    if cs.kind == "ln" and cs.opt.get("fp8"):
        return np.maximum(2.0 ** (np.floor(np.log2(np.maximum(a, 2.0 ** -6))) - 3), 2.0 ** -9)
    bits, emin = (10, -14) if cs.dtype == "f16" else (7, -126)
    return 2.0 ** (np.maximum(np.floor(np.log2(np.maximum(a, 2.0 ** -140))), emin) - bits)


def figures(got, ref, cs, mask=None):
    """(worst error / bound, share of elements != want, largest fp32 slack / output ulp) of one launch."""
    n, ratio = compare(got, ref, mask)
    m = np.ones(ref.want.shape, bool) if mask is None else mask
    return ratio, float((np.asarray(got, np.float64) != ref.want)[m].mean()), float((ref.slack / ulp_of(ref.want, cs))[m].max())


def worst(got, ref):
    got = np.asarray(got, np.float64)
    err = np.where(np.isfinite(got), np.abs(got - ref.want), np.inf) - ref.bound
    i = np.unravel_index(int(np.argmax(err)), err.shape)
    return dict(at=tuple(int(t) for t in i), got=float(got[i]), want=float(ref.want[i]), lo=float(ref.lo[i]), hi=float(ref.hi[i]))
