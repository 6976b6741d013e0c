"""fp64 restatement of what a GEMM / conv launch does BESIDE its matrix product: the LayerNorm fold of the consumer (`ln_in`), the
LayerNorm partials (`ln_out`) and GroupNorm partials (`gn_out`) a producer leaves, with bounds derived from the number formats, the
fp32 stand-ins of those paths with their mutants, the acceptance tables (which build takes which pointer) and the seeded cases of
tests/test_gemm_fused_ref_cpu.py and tests/test_gemm_fused_every_build_gpu.py.  Plain helper beside tests/gemm_conv_ref.py (the
vocabulary is that module's); no GPU use.  u = 2^-24, g(k) = k u / (1 - k u) for a chain of k fp32 operations; fused and unfused
multiply-adds are both covered by counting every multiply and every add; products of u-sized terms by SECOND = 1 + 2^-9.

`ln_in` (consumer).  `gemm_conv_ref.reference("gemm", spec)` with `ln_in = (partials (parts, M, 2) fp32, colsum (N,) fp32, eps)`
calls `ln_fold` here.  The partials and the column sums are INPUTS, exact as the fp32 values given.  In fp64, per row:
    cols = K / parts,  mean = (sum_j mean_j) / parts,  var = (sum_j M2_j + cols sum_j (mean_j - mean)^2) / K,  rstd = (var + eps)^-1/2
    x = rstd (a w^T) - rstd mean colsum + bias              (then the activation, GEGLU, residual, roundings of `reference`)
The kernel (`ln_row_stat` of gemm_geo.h, its twin in gemm_kernel, `epi_affine`) forms fmaf(acc', rstd', fmaf(-rstd' mean', colsum,
bias)).  Its shift against x, term by term:
    2 g S rstd                         the accumulation (any order of the K products, g = K u, S = sum_k |a w|), doubled as in
                                       gemm_conv_ref for the fp8 scale product and the other few-u steps of the epilogue
    u (|rstd acc| + |rstd mean colsum| + |inner| + |x|)
                                       one fp32 rounding each: the product rstd acc where the outer fma is not fused, rs.y = -rstd mean
                                       (carried to the output by |colsum|), the inner fma, the outer fma
    e_mean rstd |colsum|               e_mean = (g(parts - 1) + 3 u) mean_j |mean_j|: parts - 1 adds, 1 / parts (a division: 2 u), the product
    rho |rstd (acc - mean colsum)|     the relative error of rstd', which multiplies BOTH terms.  d_j' = mean_j - mean' is off by
                                       e_d = e_mean + u (|d_j| + e_mean) -- the cancellation when |mean| >> spread: e_mean grows with |mean|,
                                       d_j does not -- so  e_var = (g(parts - 1) + 8 u) var + cols sum_j (2 |d_j| e_d + e_d^2) / K
                                       (the sums of M2_j and d_j^2, * cols, +, * 1/parts, / cols);  r = e_var / (var + eps) + u;
                                       rho = (1 - r)^-1/2 - 1 + C_RSQRT
C_RSQRT.  What `rsqrtf` compiles to (v_rsq_f32 with or without a refinement step) cannot be derived from what is on hand, so it is
treated as C_GELU is: MEASURED_C_RSQRT is the largest (|got - want| - bound) / |rstd (acc - mean colsum)| L over the elements of the
kernels' outputs that lie outside the bound taken with the term at 0, measured against this fp64 reference on one MI355X on the
tile = 0 launches of the GPU file (`test_rsqrt_term_is_measured_at_tile_0`: fp16, bf16 and fp8 weights, cases (a) and (b), plain and
GEGLU, parts 1 / 4 / 5 / 8: 48 launches); no element of any of them lay outside, so the excess is not
positive: MEASURED_C_RSQRT = 0 and C_RSQRT = 2 x that = 0.  A v_rsq_f32 within an ulp (2 u, what tests/norm_ref.py assumes) is
1.2e-7 of |rstd (acc - mean colsum)| and disappears in 2 g S rstd (7.6e-5 of S rstd at K = 640).  No other term is measured.

`ln_out` (producer).  The reference is taken from the launch's OWN stored output x (exact fp16 / bf16 values): per row and BN-column
tile the fp64 (mean, M2), layout [N / BN][M].  The kernel sums chunks of 8 (7 adds of values <= 8 A, A = max |x| of the tile row:
|mu_c' - mu_c| <= e_c = g(7) A; the multiplication by 1/8 is exact), q_c = sum (x - mu_c')^2 = M2_c + 8 (mu_c' - mu_c)^2 up to
g(8) + 3 u relative, and merges the CPR = BN / 8 chunks in order with constant weights.  As in norm_ref's `chan_merge`: the error
of the inputs does not grow, each merge adds 3 u |d| w + u |mean| <= u (A + 6 D), D = max |x - mean|:
    e_mean = g(7) A + (CPR - 1) u (A + 6 D)                                                   (absolute, in units of u A)
    e_M2   = (g(8) + 12 u + 2 (CPR - 1) u) M2 + BN e_c^2 + 2 sqrt(BN M2) e_d + BN e_d^2,   e_d = 2 e_mean + 2 u D
(relative to M2: the leaf sums, two adds per merge, six roundings on each w2 d^2; the cross term: a mean off by e_d moves w2 d^2
by w2 (2 |d| e_d + e_d^2), sum w2 <= BN, Cauchy-Schwarz on sum w2 |d|).  A constant tile row has every chunk sum exact (8 c has 14
significant bits), so mean = c and M2 = 0 exactly: the GPU file asserts that on its own.

`gn_out` (producer, GEMM and conv).  From the stored output again: fp64 (mean, M2) per 64-row slab and channel, layout [M / 64][N]
(conv: 64 consecutive output rows of one image).  A thread holds the rows rg, rg + RG, ... of a slab (cnt = ceil(64 / RG) at most)
about its first sample, exactly the per-thread form of norm_ref:  e_t = (g(cnt) + 4 u) 2 D + u A,  (3 g(cnt) + 8 u) cnt (2 D)^2 on
its M2; one thread per column then merges the RG row groups in order with UNEQUAL counts (nb / tot is a division: 4 u |d| w + u |mean|):
    e_mean = e_t + (RG - 1) u (A + 8 D)
    e_M2   = (3 g(cnt) + 8 u) 256 D^2 + (2 (RG - 1) + 8) u M2 + 2 sqrt(64 M2) e_d + 64 e_d^2,   e_d = 2 e_mean + 2 u D
RG = threads per slab / (BN / 8) is the build's (`gn_layout`).  A constant channel is exact (d = 0 throughout).

`c_fp8` needs no reference: the bytes are `to_e4m3` of the fp16 output of the same build and case.

Room left, one MI355X, the outputs of the kernels over all cases of tests/test_gemm_fused_every_build_gpu.py (100 tests, 3.6 s wall
in the file inside the whole suite, 5.3 s alone), as that file prints them and profiles/gemm_fused_every_build.log records them per launch:
                          launches   elements     != want    largest err / bound: kernel    fp32 stand-in
  ln_in   fp16            257        42 823 040    2.3 %     0.5                            0.5
          bf16             96        15 425 280    0.3 %     1.0                            1.0
          fp8 weights     112        17 996 160   15.5 %     0.5                            0.5
  ln_in   chained, K 320    2           327 680    1.0 %     1.0                            1.0
  ln_out  fp16             65           343 040   74.9 %     0.159                          0.159
          bf16             25           168 960   67.5 %     0.140                          0.140
          fp8 weights      20           143 360   67.8 %     0.171                          0.171
  gn_out  fp16            105         1 075 200   73.3 %     0.164                          0.164
          bf16             45           460 800   73.0 %     0.165                          0.165
  gn_out -> groupnorm     150        49 152 000    0.0 %     1.0  (norm_ref's bound)        -
  c_fp8                    16         3 932 160    0          -                              -
No element outside a bound, no partial left unwritten, no stray write, every statistics launch bit-equal to its twin.  The
stand-ins follow the kernels' operation order, and on the statistics they give the kernels' figures digit for digit; a sixth of
the bound is used there (a worst-case chain of roundings that in fact average out).  The `ln_in` bound at K = 640 is the loose
one: 2 g S rstd is the worst case of any summation order, and rows a hundred spreads from zero carry S = |mean| sum |w| into it;
the kernels use half of it (fp16) or one whole admitted output step (bf16, and fp16 at K = 320).  What it still tells apart is
shown by the mutants of tests/test_gemm_fused_ref_cpu.py.
"""
import collections
import functools

import numpy as np
import torch
import torch.nn.functional as F

import gemm_conv_ref as R
from golden import make_gemm_conv_bits as maker

U = 2.0 ** -24
SECOND = 1.0 + 2.0 ** -9
F32 = np.float32
LN_EPS = 1e-5

MEASURED_C_RSQRT = 0.0          # largest excess over the bound taken with the term at 0, tile-0 launches: none (see the docstring)
C_RSQRT = 2 * MEASURED_C_RSQRT


def g_(k):
    return k * U / (1.0 - k * U)


# ---- which build takes which pointer -----------------------------------------------------------------------------------------------
# The LDS formulas of csrc/gemm_conv.hip restated (ring_bytes, lnp_off, ln_out_fits, gn_par, gn_out_fits); BUILDS is dispatch()'s
# switch: id -> (BM, BN, ring depth, threads, loader waves).  The statistics partials sit behind the staged output tile INSIDE the
# operand ring, so a build takes them only where lnp_off + partials <= ring:
#   ln_out  lnp_off(BM, BN) + BM * BN <= ST * (BM * 128 + BN * 128)       (fp8 weights: BN * 64)
#           256x128: 73728 + 32768 = 106496 > 98304 at 2 stages (id 26), <= 147456 at 3 (id 36).  Every other fp16 / bf16 build fits.
#           fp8 weights halve the weight share of the ring: 128x128x2 (53248 > 49152) and 128x160x2 (65536 > 53248) do not fit.
#   gn_out  lnp_off + slabs side by side * RG * BN * 8 <= ring, RG = threads per slab / (BN / 8)
#           256x128x2: 73728 + 32 * 1024 = 106496 > 98304 again (id 26); every other fp16 / bf16 build fits.  fill_gemm_geo refuses
#           gn_stats_out with fp8 weights outright.
#   The 8-wave kernel (91 / 92) refuses both (`gemm8_covers`), the paired-only id 90 the plain epilogue both need.
#   c_fp8   launch_k() asks for whole tiles and 8-byte rows only, so every all-fp8 build takes it, and 91 (`gemm8_covers`).
Build = collections.namedtuple("Build", "bm bn st nt lw")
BUILDS = {21: Build(128, 128, 2, 256, False), 31: Build(128, 128, 3, 256, False), 22: Build(128, 64, 2, 256, False),
          23: Build(64, 64, 2, 256, False), 24: Build(128, 160, 2, 256, False), 34: Build(128, 160, 3, 256, False),
          25: Build(64, 160, 2, 256, False), 35: Build(64, 160, 3, 256, False), 54: Build(128, 160, 3, 512, True),
          55: Build(64, 160, 3, 512, True), 65: Build(64, 160, 4, 512, True), 75: Build(64, 160, 2, 512, True),
          26: Build(256, 128, 2, 512, False), 36: Build(256, 128, 3, 512, False)}
FORM_IDS = {"f16": maker.F16_GEMM_IDS, "bf16": maker.BF16_IDS, "w8": maker.W8_IDS}
LN_OUT_IDS = {"f16": [21, 31, 22, 23, 24, 34, 25, 35, 54, 55, 65, 75, 36], "bf16": [21, 22, 23, 24, 25], "w8": [22, 23, 25, 35]}
GN_OUT_GEMM_IDS = {"f16": [21, 31, 22, 23, 24, 34, 25, 35, 54, 55, 65, 75, 36], "bf16": [21, 22, 23, 24, 25], "w8": []}
GN_OUT_CONV_IDS = {"f16": [21, 31, 22, 23, 24, 34, 25, 35, 54, 55, 36], "bf16": [21, 22, 23, 24, 25]}
C_FP8_IDS = maker.F8_IDS + [91]
LN_IN_IDS = {"f16": maker.F16_GEMM_IDS, "bf16": maker.BF16_IDS, "w8": maker.W8_IDS}
LN_IN_G8_IDS = [91, 92]


def ring_bytes(b, w8=False):
    return b.st * (b.bm * 128 + (b.bn * 64 if w8 else b.bn * 128))


def lnp_off(b):
    return (b.bm * (2 * b.bn + 32) + 15) // 16 * 16


def ln_out_fits(b, w8=False):
    return lnp_off(b) + b.bm * (b.bn // 8) * 8 <= ring_bytes(b, w8)


def gn_layout(b):
    """(slabs written side by side, threads per slab, row groups RG, most rows a thread holds)."""
    par = 2 if b.lw and b.bm == 128 else 1
    gnt = b.nt // par
    rg = gnt // (b.bn // 8)
    return par, gnt, rg, (64 + rg - 1) // rg


def gn_out_fits(b, w8=False):
    par, gnt, rg, _ = gn_layout(b)
    return b.bm % 64 == 0 and b.bn <= gnt and lnp_off(b) + par * rg * b.bn * 8 <= ring_bytes(b, w8)


# ---- ln_in: the fold ------------------------------------------------------------------------------------------------------------------
def ln_row_stats(part, K, eps, c_rsqrt=None):
    """fp64 merge of the partials (parts, M, 2): (mean, rstd, e_mean, rho) per row, see the module docstring."""
    c_rsqrt = C_RSQRT if c_rsqrt is None else c_rsqrt
    pt = part.double()
    parts = pt.shape[0]
    cols = K // parts
    assert parts * cols == K
    mj, qj = pt[..., 0], pt[..., 1]
    mean = mj.mean(0)
    dj = mj - mean
    var = (qj.sum(0) + cols * (dj ** 2).sum(0)) / K
    rstd = (var + eps) ** -0.5
    e_mean = (g_(parts - 1) + 3 * U) * mj.abs().mean(0)
    e_d = e_mean + U * (dj.abs() + e_mean)
    e_var = (g_(parts - 1) + 8 * U) * var + cols * (2 * dj.abs() * e_d + e_d ** 2).sum(0) / K
    r = e_var / (var + eps) + U
    assert float(r.max()) < 0.5, float(r.max())
    rho = (1 - r) ** -0.5 - 1 + c_rsqrt
    return mean, rstd, e_mean, rho


def ln_fold(s, acc, S, g):
    """acc = a w^T (times the fp8 scales), S = sum |a w|, g = K u  ->  (x before the activation, its shift)."""
    part, colsum, eps = s["ln_in"]
    K = s["a"].shape[1]
    mean, rstd, e_mean, rho = ln_row_stats(part, K, eps, s.get("c_rsqrt"))
    cs = colsum.double()[None, :]
    x0 = rstd[:, None] * acc
    t = (rstd * mean)[:, None] * cs
    bias = s["bias"].double()[None, :] if s.get("bias") is not None else torch.zeros((), dtype=torch.float64)
    inner = bias - t
    x = x0 + inner
    dx = 2 * g * S * rstd[:, None] + U * (x0.abs() + t.abs() + inner.abs() + x.abs()) + (e_mean * rstd)[:, None] * cs.abs() \
        + rho[:, None] * (x0 - t).abs()
    return x, dx * SECOND


def rsqrt_scale(spec):
    """|rstd (acc - mean colsum)| L per element of the logical output: what C_RSQRT multiplies (GEGLU: the product rule's two terms)."""
    s = dict(spec)
    part, colsum, eps = s["ln_in"]
    a, w = s["a"], s["w"]
    A, Wm = (R.to_e4m3(a), w.float().double() * s["wscale"].double()[:, None]) if s.get("wscale") is not None else (a.double(), w.double())
    mean, rstd, _, _ = ln_row_stats(part, A.shape[1], eps, 0.0)
    z = (rstd[:, None] * (A @ Wm.T - mean[:, None] * colsum.double()[None, :])).abs()
    if s.get("epi", R.EPI_PLAIN) == R.EPI_GEGLU:
        x = R.reference("gemm", dict(s, epi=R.EPI_PLAIN, act=R.ACT_NONE, res=None, c_rsqrt=0.0)).p
        val, par = R.unpair(x)
        zv, zp = R.unpair(z)
        return R.gelu(par).abs() * zv + val.abs() * 1.13 * zp
    return z * R.LIPSCHITZ[s.get("act", R.ACT_NONE)]


def exact_partials(a, parts):
    """fp32 (parts, M, 2): (mean, M2) of each of the `parts` equal column groups of the stored rows, in fp64, rounded to fp32."""
    M, K = a.shape
    z = a.double().reshape(M, parts, K // parts)
    mu = z.mean(-1)
    return torch.stack([mu, ((z - mu[..., None]) ** 2).sum(-1)], -1).permute(1, 0, 2).float().contiguous()


def rsq32(x):
    return torch.from_numpy((1.0 / np.sqrt(x.numpy().astype(np.float64))).astype(F32))


LN_IN_MUTANTS = ("index_m_parts", "clamp_off_by_one", "colsum_unrounded", "mean_as_8_parts")


def ln_in_standin(spec, mut=None):
    """A correct kernel in fp32 with the kernel's merge formulas and rounding points (`ln_row_stat`, `epi_affine`, the two
    roundings).  Mutants: index_m_parts (the partial of (j, m) read at [m][j]), clamp_off_by_one (the row clamp is M - 2: the last
    row reads its neighbour's partials), colsum_unrounded (column sums of the folded weight BEFORE its rounding, spec["w32"]),
    mean_as_8_parts (the mean divided by 8 whatever `parts` is)."""
    s = dict(spec)
    part, colsum, eps = s["ln_in"]
    dt = s["a"].dtype
    if s.get("wscale") is not None:
        acc = (R.to_e4m3(s["a"]).float() @ s["w"].float().T) * s["wscale"][None, :]
    else:
        acc = s["a"].float() @ s["w"].float().T
    M, K = s["a"].shape
    parts = part.shape[0]
    cols = K // parts
    pt = part
    if mut == "index_m_parts":
        pt = part.reshape(-1, 2)[(torch.arange(M)[None, :] * parts + torch.arange(parts)[:, None]).reshape(-1)].reshape(parts, M, 2)
    if mut == "clamp_off_by_one":
        pt = pt[:, torch.arange(M).clamp(max=M - 2)]
    if mut == "colsum_unrounded":
        colsum = s["w32"].sum(dim=1)
    mj, qj = pt[..., 0], pt[..., 1]
    sm = torch.zeros(M)
    for j in range(parts):
        sm = sm + mj[j]
    inv_p = torch.tensor(1.0) / torch.tensor(float(parts))
    mean = sm * (torch.tensor(0.125) if mut == "mean_as_8_parts" else inv_p)
    m2, dev = torch.zeros(M), torch.zeros(M)
    for j in range(parts):
        d = mj[j] - mean
        m2, dev = m2 + qj[j], dev + d * d
    var = (m2 + float(cols) * dev) * inv_p / float(cols)
    rstd = rsq32(var + torch.tensor(eps, dtype=torch.float32))
    rsy = -rstd * mean
    bias = s["bias"].float()[None, :] if s.get("bias") is not None else torch.zeros(())
    inner = (rsy[:, None].double() * colsum[None, :].double() + bias.double()).float()          # fmaf: one rounding
    v = (acc.double() * rstd[:, None].double() + inner.double()).float()
    if s.get("epi", R.EPI_PLAIN) == R.EPI_GEGLU:
        val, par = R.unpair(v)
        return (val * F.gelu(par)).to(dt).double()
    v = {R.ACT_NONE: lambda t: t, R.ACT_SILU: F.silu}[s.get("act", R.ACT_NONE)](v)
    y1 = v.to(dt).float()
    return ((y1 + s["res"].float()) if s.get("res") is not None else y1).to(dt).double()


def _ulp(w, dt):
    _, e = torch.frexp(w.float().abs().clamp_min(2.0 ** -14))
    return torch.ldexp(torch.ones(()), e - 1 - (10 if dt == torch.float16 else 7))


LN_K = 640
LN_PARTS = (1, 4, 5, 8)
LN_SHAPES = {"a": R.G1, "b": R.G2, "g8": R.G8}
ZERO_VAR_ROW = 7


def ln_in_case(form, shape, what, parts, K=LN_K):
    """The consumer with SYNTHETIC partials: the exact (mean, M2) of `parts` equal column groups of the raw rows, as fp32.
    shape: a (ragged 300 x 336: the row clamp and the element-wise write-out), b (whole tiles 512 x 640), g8 (256 x 1280, the
    8-wave kernel's).  what: full (bias + residual + SiLU), geglu (on the `pair_rows` layout), out_t (tr_from = 768, g8 only).
    Rows: spread 0.5 about a mean of +4, -4, +100, -100 spreads (row m: m % 4); row 7 is constant (zero variance: rstd = eps^-1/2).
    The folded weight: w32 is the UNROUNDED fold, 0.4 ulp above the stored weight everywhere, so that its column sums differ from
    those of the stored values by the same sign in every term (a random rounding would hide that mutant in the accumulation term);
    colsum is the fp32 sum of the STORED values, as `ops.LnFold` takes it."""
    M, N = LN_SHAPES[shape]
    g = R._gen(f"ln_in.{form}.{shape}.{what}.{parts}.{K}")
    dt = R.DTYPES.get(form, torch.float16)
    spread = 0.5
    offs = torch.tensor([4.0, -4.0, 100.0, -100.0])[torch.arange(M) % 4] * spread
    a = (torch.randn(M, K, generator=g) * spread + offs[:, None]).to(dt)
    a[ZERO_VAR_ROW] = 0.75
    gamma = 1.0 + 0.2 * torch.randn(K, generator=g)
    w = ((torch.randn(N, K, generator=g) * K ** -0.5) * gamma[None, :]).to(dt)
    spec = dict(a=R.wide(a), bias=R._rand(g, N, dtype=dt))
    if form == "w8":
        q, sc = R.quantize_fp8_rows(w)
        spec.update(w=q, wscale=sc, w32=w.float())
        colsum = (q.float().sum(dim=1) * sc).contiguous()
    else:
        spec.update(w=w, w32=w.float() + 0.4 * _ulp(w, dt))
        colsum = w.float().sum(dim=1).contiguous()
    spec["ln_in"] = (exact_partials(a, parts), colsum, LN_EPS)
    if what == "full":
        spec.update(res=R._res(g, M, N, spec["bias"], dt), act=R.ACT_SILU)
    elif what == "geglu":
        spec.update(epi=R.EPI_GEGLU)
    elif what == "out_t":
        spec.update(out_t=768)
    else:
        raise ValueError(what)
    return R.Case("gemm", spec)


@functools.lru_cache(maxsize=None)
def ln_in_cases(form):
    """name -> Case for the 4-wave builds of `form`."""
    return {f"{sh}.{what}.p{p}": ln_in_case(form, sh, what, p) for sh in ("a", "b") for what in ("full", "geglu") for p in LN_PARTS}


@functools.lru_cache(maxsize=None)
def ln_in_g8_cases():
    out = {f"g8.{what}.p{p}": ln_in_case("f16", "g8", what, p) for what in ("full", "geglu") for p in LN_PARTS}
    out["g8.out_t.p5"] = ln_in_case("f16", "g8", "out_t", 5)
    return out


# ---- ln_out / gn_out: statistics of the stored values -----------------------------------------------------------------------------------
Stats = collections.namedtuple("Stats", "mean m2 e_mean e_m2")


def ln_out_reference(x, bn):
    """x (M, N) float64, the stored output -> Stats in layout [N / BN][M]."""
    M, N = x.shape
    cpr = bn // 8
    z = x.reshape(M, N // bn, bn)
    mean = z.mean(-1)
    dev = z - mean[..., None]
    m2 = (dev ** 2).sum(-1)
    A, D = z.abs().amax(-1), dev.abs().amax(-1)
    e_c = g_(7) * A
    e_mean = e_c + (cpr - 1) * U * (A + 6 * D)
    e_d = 2 * e_mean + 2 * U * D
    e_m2 = (g_(8) + 12 * U + 2 * (cpr - 1) * U) * m2 + bn * e_c ** 2 + 2 * (bn * m2).sqrt() * e_d + bn * e_d ** 2
    return Stats(mean.T, m2.T, (e_mean * SECOND).T, (e_m2 * SECOND + 2.0 ** -149).T)


def gn_out_reference(x, rg):
    """x (M, N) float64, the stored output in logical row order; rg = row groups of the build -> Stats in layout [M / 64][N]."""
    M, N = x.shape
    cnt = (64 + rg - 1) // rg
    z = x.reshape(M // 64, 64, N)
    mean = z.mean(1)
    dev = z - mean[:, None]
    m2 = (dev ** 2).sum(1)
    A, D = z.abs().amax(1), dev.abs().amax(1)
    e_mean = (g_(cnt) + 4 * U) * 2 * D + U * A + (rg - 1) * U * (A + 8 * D)
    e_d = 2 * e_mean + 2 * U * D
    e_m2 = (3 * g_(cnt) + 8 * U) * 256 * D ** 2 + (2 * (rg - 1) + 8) * U * m2 + 2 * (64 * m2).sqrt() * e_d + 64 * e_d ** 2
    return Stats(mean, m2, e_mean * SECOND, e_m2 * SECOND + 2.0 ** -149)


def stats_compare(got, ref):
    """got: fp32 (..., 2) in the layout of `ref`.  -> (elements outside, largest err / bound over mean and M2, worst as text)."""
    gm, gq = got[..., 0].double(), got[..., 1].double()
    n1, w1 = R.compare(gm, ref.mean, ref.e_mean)
    n2, w2 = R.compare(gq, ref.m2, ref.e_m2)
    with np.errstate(all="ignore"):
        room = max(_ratio(gm, ref.mean, ref.e_mean), _ratio(gq, ref.m2, ref.e_m2))
    return n1 + n2, room, f"mean {w1} M2 {w2}"


def _ratio(got, want, bound):
    err = (got - want).abs()
    q = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(q.max())


def _fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


STAT_MUTANTS_LN = ("unrounded", "before_res", "sum_of_squares", "index_m_parts")
STAT_MUTANTS_GN = ("unrounded", "before_res", "sum_of_squares", "short_group_as_full", "half_slab")


def ln_out_standin(x, bn, mut=None):
    """The fast write-out's statistics on fp32 values x (M, N): chunk sums of 8, mean, squared deviations by fma, then the
    fixed-order merge with constant weights.  -> fp32 (N / BN, M, 2).  Mutants: sum_of_squares (M2 = sum x^2), index_m_parts (the
    buffer written as [M][N / BN]); `unrounded` / `before_res` are the caller's choice of x."""
    x = np.ascontiguousarray(x, dtype=F32)
    M, N = x.shape
    T, cpr = N // bn, bn // 8
    c = x.reshape(M, T, cpr, 8)
    s = c[..., 0]
    for t in range(1, 8):
        s = s + c[..., t]
    mu = s * F32(0.125)
    q = np.zeros_like(mu)
    for t in range(8):
        d = c[..., t] - (F32(0) if mut == "sum_of_squares" else mu)
        q = _fma32(d, d, q)
    mean, m2 = mu[..., 0], q[..., 0]
    for j in range(1, cpr):
        d = mu[..., j] - mean
        mean = mean + d * (F32(1) / F32(j + 1))
        m2 = m2 + (q[..., j] + (F32(0) if mut == "sum_of_squares" else d * d * (F32(8) * F32(j) / F32(j + 1))))
    out = np.stack([mean, m2], -1)          # [M][T]
    if mut == "index_m_parts":
        return torch.from_numpy(np.ascontiguousarray(out.reshape(-1, 2)).reshape(T, M, 2))
    return torch.from_numpy(np.ascontiguousarray(out.transpose(1, 0, 2)))


def gn_out_standin(x, rg, mut=None):
    """The GroupNorm write-out on fp32 values x (M, N): per thread the rows rg, rg + RG, ... of a slab about the first one, then
    the merge of the RG row groups in order with their counts.  -> fp32 (M / 64, N, 2).  Mutants: sum_of_squares,
    short_group_as_full (every row group weighted as ceil(64 / RG) rows), half_slab (slabs start at row 32)."""
    x = np.ascontiguousarray(x, dtype=F32)
    if mut == "half_slab":
        x = np.roll(x, -32, axis=0)
    M, N = x.shape
    z = x.reshape(M // 64, 64, N)
    if mut == "sum_of_squares":
        mean = z.mean(1, dtype=np.float64).astype(F32)
        return torch.from_numpy(np.stack([mean, (z * z).sum(1, dtype=F32)], -1))
    n, mean, m2 = F32(0), np.zeros((M // 64, N), F32), np.zeros((M // 64, N), F32)
    for q in range(rg):
        rows = z[:, q::rg]
        cnt = rows.shape[1]
        k0 = rows[:, 0]
        s8, q8 = np.zeros_like(k0), np.zeros_like(k0)
        for j in range(cnt):
            d = rows[:, j] - k0
            s8, q8 = s8 + d, _fma32(d, d, q8)
        inv = F32(1) / F32(cnt)
        pm, pq = k0 + s8 * inv, np.maximum(q8 - s8 * s8 * inv, F32(0))
        nb = F32((64 + rg - 1) // rg) if mut == "short_group_as_full" else F32(cnt)
        tot = n + nb
        d = pm - mean
        mean = mean + d * (nb / tot)
        m2 = m2 + (pq + d * d * (n * nb / tot))
        n = tot
    return torch.from_numpy(np.stack([mean, m2], -1))


# ---- the producers' cases ---------------------------------------------------------------------------------------------------------------
PM, PN, PK = 512, 640, 320          # the whole-tile GEMM of gemm_conv_ref (case b); two "images" of 256 rows for the row bias
CONST_COLS = 320                    # weight rows [0, 320) zeroed: whole column tiles of every BN (5 x 64, 2 x 160, 2 of 128 and a half)
CONST_CH = 37


def producer_case(form, op, what):
    """Plain epilogue, bias (+ residual): what every statistics launch runs.
    op: gemm (512 x 640 x 320), conv (R = 2, 16 x 16, Cin 64 -> Cout 640), conv2 (the same from 32 x 32 with stride 2).
    what: res (bias + residual), rowmean (residual rows about +-100 spreads), const (weight rows [0, 320) zero, a constant bias
    there, no residual: constant row tiles), chanoff (channel offsets of about 100 spreads), constch (channel 37: zero weight row,
    constant residual column), rowbias (a row bias per image of 256 rows)."""
    g = R._gen(f"producer.{form}.{op}.{what}")
    dt = R.DTYPES.get(form, torch.float16)
    N = PN
    bias = R._rand(g, N, dtype=dt)
    if op == "gemm":
        M = PM
        w = R._rand(g, N, PK, scale=PK ** -0.5, dtype=dt)
        spec = dict(a=R.wide(R._rand(g, M, PK, dtype=dt)))
    else:
        H = 32 if op == "conv2" else 16
        M = 2 * 256
        w = R._rand(g, N, 3, 3, 64, scale=576 ** -0.5, dtype=dt)
        spec = dict(x=R.wide(R._rand(g, 2, H, H, 64, dtype=dt), 64), ksize=3, stride=2 if op == "conv2" else 1, upsample=False, pad_mode=0)
    noise = 0.5 * torch.randn(M, N, generator=g)
    res = None
    if what == "res":
        res = noise - bias.float()[None, :]
    elif what == "rowmean":
        res = noise + (torch.tensor([150.0, -150.0])[torch.arange(M) % 2])[:, None]
    elif what == "const":
        w[:CONST_COLS] = 0
        bias[:CONST_COLS] = 0.8125
    elif what == "chanoff":
        res = noise + (110.0 * ((torch.arange(N) % 5) - 2.0) / 2.0)[None, :]
    elif what == "constch":
        w[CONST_CH] = 0
        res = noise
        res[:, CONST_CH] = 1.25
    elif what == "rowbias":
        res = noise
        spec.update(rowbias=R._rand(g, 2, N, dtype=dt), rows_per_rb=256)
    else:
        raise ValueError(what)
    if form == "w8":
        spec["w"], spec["wscale"] = R.quantize_fp8_rows(w)
    else:
        spec["w"] = w
    spec["bias"] = bias
    if res is not None:
        spec["res"] = res.to(dt)
    return R.Case("gemm" if op == "gemm" else "conv", spec)


LN_OUT_WHATS = ("res", "rowmean", "const")
GN_OUT_WHATS = ("chanoff", "constch", "rowbias")


@functools.lru_cache(maxsize=None)
def producer_cases(form, op):
    whats = (LN_OUT_WHATS if op == "gemm" else ()) + GN_OUT_WHATS
    return {w: producer_case(form, op, w) for w in whats}


def producer_standin(case):
    """A correct plain-epilogue kernel in fp32 -> (the fp32 value before the last rounding, y1 as fp32, the stored values as fp32)."""
    kind, s = case
    dt = (s["a"] if kind == "gemm" else s["x"]).dtype
    if kind == "conv":
        v = R.im2col(s["x"], s["ksize"], s["stride"], s["upsample"], s["pad_mode"]).float() @ s["w"].float().reshape(s["w"].shape[0], -1).T
    elif s.get("wscale") is not None:
        v = (R.to_e4m3(s["a"]).float() @ s["w"].float().T) * s["wscale"][None, :]
    else:
        v = s["a"].float() @ s["w"].float().T
    v = v + s["bias"].float()[None, :]
    if s.get("rowbias") is not None:
        v = v + s["rowbias"].float()[torch.arange(v.shape[0]) // s["rows_per_rb"]]
    y1 = v.to(dt).float()
    pre = y1 + s["res"].float() if s.get("res") is not None else v
    return pre, y1, pre.to(dt).float()


def chain_case(form):
    """Producer -> consumer at tile = 0: 256 x 320 x 320 (bias + residual rows about 4 spreads from 0; the chooser's 64 x 64 tile
    leaves 5 partials) into 256 x 640 x 320 with the LayerNorm folded in.  -> (producer Case, gamma, beta, weight, bias) on the CPU."""
    g = R._gen(f"chain.{form}")
    dt = R.DTYPES[form]
    M, C, N = 256, 320, 640
    res = (0.5 * torch.randn(M, C, generator=g) + 2.0 * torch.randn(M, 1, generator=g)).to(dt)
    prod = R.Case("gemm", dict(a=R.wide(R._rand(g, M, C, dtype=dt)), w=R._rand(g, C, C, scale=C ** -0.5, dtype=dt), bias=R._rand(g, C, dtype=dt), res=res))
    gamma, beta = (1.0 + 0.2 * torch.randn(C, generator=g)).to(dt), (0.3 * torch.randn(C, generator=g)).to(dt)
    return prod, gamma, beta, R._rand(g, N, C, scale=C ** -0.5, dtype=dt), R._rand(g, N, dtype=dt)


# ---- the log ---------------------------------------------------------------------------------------------------------------------------
LOG_HEADER = "# case | build | elements | != want | kernel err/bound | stand-in err/bound | ms"


def log_line(case, build, elements, differ, kernel, standin, ms):
    f = lambda v: "-" if v is None else f"{v:.5f}"
    return f"{case} | {build} | {elements} | {differ} | {f(kernel)} | {f(standin)} | {ms:.1f}"
