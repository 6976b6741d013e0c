"""fp64 restatement of one `ops.gemm(..., epi=EPI_XATTN, xattn=(segs, Tq))` launch -- `attn2.to_q` plus the text and IP
cross-attention of TA_IPAttnProcessor2_0 in one launch: the `if (g.xa_on)` block of `gemm_kernel<64,128,...>` in csrc/gemm_conv.hip,
dispatch id 93 -- with a per-element interval derived from the number formats, the fp32 stand-in of that block with its mutants,
and the seeded cases of tests/test_xattn_ref_cpu.py and tests/test_xattn_every_case_gpu.py.  Plain helper; no GPU use.  Built
from tests/gemm_conv_ref.py (the q projection and its admitted interval), tests/gemm_fused_ref.py (the LayerNorm fold) and the
constants of tests/attention_ref.py.

`reference(case)` returns a `Ref` in the layout of the O view, (R * Tq, heads * 64) float64: `want`, `lo`, `hi`,
`bound = max(hi - want, want - lo)`, `value` and `shift` (before the output rounding), `q` and `dq` (the projection as the
attention part takes it, and the half-width of its admitted interval).  `reference(..., rounding=False)` drops every rounding
point: plain softmax(q k^T) v of the unrounded projection, summed over the two segments.

Rounding points (the ones the kernel's code shows, no others; csrc/gemm_conv.hip)
  q       fp16: `qf[i][j >> 1][..] = (E)iir::epi_affine(acc, rs, colsum, bias)` -- "what the plain epilogue would have stored":
          a @ w.T + bias, or with `ln_in` the LayerNorm fold rstd * (a w^T - mean colsum) + bias.  `gemm_conv_ref.reference("gemm",
          spec)` gives its value p, its shift d and so the admitted fp16 interval [round(p - d), round(p + d)] of every q element
          (`Ref.lo`, `Ref.hi`); q = round(p) is the reference's.  q carries scale x log2 e (as `q_prescaled` of ops.attention).
  P       fp16, AFTER the normalisation: `pf[i][kp][t] = (E)(sa[i][ka][t] * sm[..])`, sm = `__builtin_amdgcn_rcpf` of the
          segment's fp32 sum of p = `__builtin_amdgcn_exp2f(s - max)`.  Scores, maxima, p and sums stay fp32.
  O       fp16, ONCE: both segments' P V accumulate in the same fp32 accumulators (`acc[i][j] = mfma16(vf, pf[i][kp], acc[i][j])`,
          kp = 0..4 runs over text and IP key columns alike) and leave through the plain epilogue's `(E)iir::rounded_f32(a[t])`.
          (The d64 attention kernel holds its first segment as fp16, `ohold` of tests/attention_ref.py; this kernel does not.)
  out_scale  phase 2 of the write-out multiplies the stored fp16 tile: `o[k][t] = (E)((float)v[t] * g.out_scale)`, a second fp16
          rounding of round(O) * out_scale.  That is a coherent scaling of the finished output; `ops.gemm` documents it.

The interval.  Per image, head, query row and segment let s_j = q . k_j (fp64, log2 units), P = softmax_2(s) over keys [0, Tkv),
u = 2^-24.  What the kernel holds differs from that by

  the q interval       dq = max(hi_q - q, q - lo_q) per element.  A q off by dq moves score j by at most sum_d |dq_d| |k_jd|; a
                       shift common to all keys of a row leaves the softmax alone, so it also moves the scores RELATIVE to key 0
                       by at most sum_d |dq_d| |k_jd - k_0d|.  Dq = the smaller of the two maxima over j (the second is 0 when
                       all keys of a segment are equal).
  the fp32 score chain ds = (D + KS + 2) u S, D = 64, KS = 2 chained MFMAs per score, S = max_j sum_d (|q_d| + dq_d) |k_jd|: D for
                       the fp32 accumulation of the 64 exact fp16 products in any order, KS for the chain, 2 for `s - max`
                       (|s - max| <= 2 S).  The maximum itself is exact (a selection).
  =>                   every score moves by at most Dq + ds, every ratio p_j / p_i by a factor in [2^-L, 2^L], L = 2 (Dq + ds), so
                       P_j in [P / (P + (1 - P) 2^L),  P / (P + (1 - P) 2^-L)]  (the odds of key j against the rest move by 2^+-L).
                       This lies inside the simpler [P 2^-L, P 2^L] -- O moves by at most (2^L - 1) (P @ |V|) -- and does not
                       admit P > 1 on a row that one key dominates.
  v_exp_f32, v_rcp_f32 E_EXP on numerator and denominator (attention_ref.E_EXP = 2^-23: 1 ulp ASSUMED, NOBODY MEASURED IT) and
                       E_RCP = 2^-23 for the reciprocal (1 ulp, ASSUMED likewise); one u for the product p * (1 / sum).
  the fp32 sum         Tkv u: the segment's sum of at most 80 / 64 non-negative terms, any order (lane sums, two shuffles).
  =>                   P' in [P_lo (1 - e1), P_hi (1 + e1)],  e1 = 2 E_EXP + E_RCP + (Tkv + 1) u.
  the fp16 rounding of P, and P underflow
                       pf in [round16(P'_lo), round16(P'_hi)]: the image of the interval under the (monotone) rounding, subnormals
                       and 0 included -- a P below 2^-14 is rounded absolutely (2^-25 per key), one below 2^-25 is 0, and an exp2
                       that underflows in fp32 has long been 0 in fp16.  Where no rounding boundary lies inside, the two ends are
                       the same fp16 number and P is pinned exactly.
  P V                  value = sum_j round16(P_j) v_j over both segments; the ends  sum_j min / max (pf_lo v_j, pf_hi v_j)  -+
                       (Tkv_text + Tkv_ip + 5) u (pf_hi @ |V|): the fp32 accumulation of the exact fp16 products of both segments
                       in any order, 5 chained MFMAs.  Masked keys and pad columns carry pf = 0 exactly and add nothing.
  `lo` / `hi`          the images of these ends under the output rounding(s), as in the other references; no closed form
                       u |want| + shift.  `shift` = the larger distance of an end from `value`.
Nothing here comes from a kernel's output; no term is measured.  Assumed, not measured: E_EXP and E_RCP.

`standin(case, mut=None)`: the block in fp32 torch with its staging (the 144-row K image: text keys at rows [0, 80), IP keys at
[80, 144), rows past Tkv repeating the last key; the V^T image of 10 + 8 chunks of 8 keys, chunks past roundup8(Tkv) / 8
repeating the last one), its masks and its three rounding points.  MUTANTS each model one realistic error; the CPU file names
the case that catches each.

Room left, one MI355X, the kernel's outputs over all cases of tests/test_xattn_every_case_gpu.py, as that file prints them
and profiles/xattn_every_case.log records them per case:
  14 cases, 101 launches, 319 488 elements: 0 outside [lo, hi]; 0.71 % differ from `want` (per case 0 to 4.1 %: the most where
  the LayerNorm fold widens the q interval; 0 in the `equal` cases and at Tkv = (1, 1), where lo = hi for most elements and the
  kernel had to store exactly that value); largest |got - want| / bound 1.0 for the kernel and 1.0 for the fp32 stand-in (a whole
  admitted step: by construction the ratio cannot say more); 2.3 s for the file run alone (0.4 s from its first case to its last).  Every bit contract of the GPU file held.  The
  kernel's own error is far inside the interval where the q term is wide (0.02 of the bound at K = 192 with the fold): that
  term is the worst case of ANY summation order of the projection carried through the softmax, and is
  the loose part of this bound; what it still tells apart is shown by the mutants of tests/test_xattn_ref_cpu.py.
"""
import collections
import functools

import torch

import gemm_conv_ref as G
import gemm_fused_ref as F
from attention_ref import BORDER, E_EXP, PAD_V, SENTINEL, r16, roundup8

D = 64
KROWS_TEXT, KROWS_IP = 80, 64          # the K image: 144 rows; the V^T image: 10 + 8 chunks of 8 keys
KS = 2
U = 2.0 ** -24
E_RCP = 2.0 ** -23                     # assumed: 1 ulp of fp32 (v_rcp_f32), not measured
MARGIN = 30.0
SPARE_ROWS = 3

Case = collections.namedtuple("Case", "name R Tq heads K tk fold bias regime out_scale")
Ops = collections.namedtuple("Ops", "spec kv bufs plants")          # spec: the GEMM reference's; kv: [(k view, rows, vt view, vbs, Tkv)] x 2
Ref = collections.namedtuple("Ref", "want lo hi bound value shift q dq")


def case(name, R, Tq, heads, K, tk, fold=0, bias=True, regime="flat", out_scale=1.0):
    """fold: 0 or the number of LayerNorm partials.  regime: flat / plant / big / equal (see `operands`)."""
    return Case(name, R, Tq, heads, K, tuple(tk), fold, bias, regime, float(out_scale))


def _gen(name):
    return torch.Generator().manual_seed(int.from_bytes(name.encode(), "little") % (2 ** 31 - 1))


def heads_of(x, cs):
    """(R * Tq, heads * 64) -> (R, heads, Tq, 64)."""
    return x.reshape(cs.R, cs.Tq, cs.heads, D).permute(0, 2, 1, 3)


def to_o_layout(x):
    R, H, T, d = x.shape
    return x.permute(0, 2, 1, 3).reshape(R * T, H * d)


def k_tiles(cs):
    return cs.K // 64


def tiles_per_image(cs):
    return cs.Tq // 64


def head_tiles(cs):
    return cs.heads // 2


# ---- operands ---------------------------------------------------------------------------------------------------------------------------
def _framed(t, fill=float("nan"), rows=1, cols=BORDER):
    """The same values as a view inside a `fill`-filled buffer: `rows` spare rows above and below, `cols` columns on either side
    (2-D), or `cols` elements on either side (1-D).  -> (view, whole buffer)."""
    if t.dim() == 1:
        big = torch.full((t.numel() + 2 * cols,), fill, dtype=t.dtype)
        big[cols:cols + t.numel()] = t
        return big[cols:cols + t.numel()], big
    big = torch.full((t.shape[0] + 2 * rows, t.shape[1] + 2 * cols), fill, dtype=t.dtype)
    big[rows:rows + t.shape[0], cols:cols + t.shape[1]] = t
    return big[rows:rows + t.shape[0], cols:cols + t.shape[1]], big


def _kv_heads(cs, kv):
    """Per segment K (R, H, Tkv, 64) and V (R, H, Tkv, 64) as float64, read from the views by their strides."""
    out = []
    for kview, rows, vt, vbs, tkv in kv:
        K = torch.stack([kview[b * rows:b * rows + tkv] for b in range(cs.R)]).reshape(cs.R, tkv, cs.heads, D).permute(0, 2, 1, 3)
        V = torch.stack([vt[:, b * vbs:b * vbs + tkv].reshape(cs.heads, D, tkv).permute(0, 2, 1) for b in range(cs.R)])
        out.append((K.double(), V.double(), tkv))
    return out


def plant_list(cs):
    """(row, segment, key): the first and the last key of each segment that has more than one key, each in a row of its own."""
    out, row = [], 1
    for sg, t in enumerate(cs.tk):
        if t > 1:
            out += [(row, sg, 0), (row + 1, sg, t - 1)]
        row += 2
    return tuple(out)


def margins(cs, ops, q):
    """For every plant the smallest margin (log2 units, fp64, over images and heads) of the planted key over every other key of
    its segment, from the operands as stored and the fp16 q."""
    qh = heads_of(q, cs)
    segs = _kv_heads(cs, ops.kv)
    out = []
    for row, sg, key in ops.plants:
        s = (qh[:, :, row:row + 1] @ segs[sg][0].transpose(-1, -2))[:, :, 0]
        top = s[..., key].clone()
        s[..., key] = -float("inf")
        out.append(float((top - s.max(-1).values).min()))
    return out


@functools.lru_cache(maxsize=None)
def operands(cs):
    """The launch of `cs` as the GPU file issues it, on the CPU.  Every operand is a view of a wider buffer: `a` (lda = K + 16,
    a NaN row above and below), `w` a contiguous row slice between NaN rows, bias / colsum slices of longer vectors; K a column
    slice (ldk = C + 16, NaN beside it) with `rows` = Tkv + 5 rows per image and NaN in the rows past Tkv; V^T a row slice with
    NaN rows beside the heads, vt_batch_stride = roundup8(Tkv) + 16, NaN outside every image's window and +-1000 on
    [Tkv, roundup8(Tkv)).  (The O buffer is made by the GPU file.)
    Regimes.  flat: scores of standard deviation 1 (q elements ~ 1/8, k ~ 1).  plant: flat, and `plant_list` keys set to beta q
    of their row so that they win by >= 30 log2 units (checked in fp64 on the stored values: `margins`).  big: k ~ 200, scores
    of magnitude ~200, so the maximum subtraction matters and one segment's maximum lies far from the other's.  equal: all keys
    of a segment and image are one (small) row, so P = 1 / Tkv exactly and O = mean of V; V = 1 + noise / 4, so P @ |V| = |O|.
    With `fold` the rows of `a` have spread 0.5 about a mean of +-2 / +-20 spreads (row m: m % 4) and the partials are their exact
    (mean, M2) as fp32 inputs.  (The fold's shift grows with |mean| sum |w|, so the q interval, and with it the interval of O, is
    wide on the +-20 rows and narrow on the +-2 rows: both kinds are in every fold case.)"""
    g = _gen("xattn." + cs.name)
    R, Tq, H, K = cs.R, cs.Tq, cs.heads, cs.K
    M, C = R * Tq, H * D
    if cs.fold:
        offs = torch.tensor([2.0, -2.0, 20.0, -20.0])[torch.arange(M) % 4] * 0.5
        a = (torch.randn(M, K, generator=g) * 0.5 + offs[:, None]).half()
        gamma = 1.0 + 0.2 * torch.randn(K, generator=g)
        w = (torch.randn(C, K, generator=g) * (K ** -0.5 / 8) * gamma[None, :]).half()
    else:
        a = torch.randn(M, K, generator=g).half()
        w = (torch.randn(C, K, generator=g) * (K ** -0.5 / 8)).half()
    av, ab = _framed(a)
    wv, wb = _framed(w, cols=0)
    spec, bufs = dict(a=av, w=wv), [ab, wb]
    if cs.bias:
        spec["bias"], bb = _framed((torch.randn(C, generator=g) * (0.3 / 8)).half())
        bufs.append(bb)
    if cs.fold:
        colsum, cb = _framed(w.float().sum(dim=1), cols=4)
        part = F.exact_partials(av, cs.fold)
        spec["ln_in"] = (part, colsum, F.LN_EPS)
        bufs += [cb, part]
    sig_k = {"big": 200.0, "equal": 2.0 ** -5}.get(cs.regime, 1.0)
    ks, vs = [], []
    for t in cs.tk:
        k = torch.randn(R, t, C, generator=g) * sig_k
        v = torch.randn(R, t, C, generator=g)
        if cs.regime == "equal":
            k, v = k[:, :1].expand(-1, t, -1), 1.0 + 0.25 * v
        ks.append(k.half().clone())
        vs.append(v.half())
    plants = plant_list(cs) if cs.regime == "plant" else ()

    def pack():
        kv, kb_all = [], []
        for k, v, tkv in zip(ks, vs, cs.tk):
            rows, vbs, tpad = tkv + 5, roundup8(tkv) + 16, roundup8(tkv)
            kb = torch.full((R * rows, C + 2 * BORDER), float("nan"), dtype=torch.half)
            vb = torch.full((C + 2 * BORDER, R * vbs + 64), float("nan"), dtype=torch.half)
            for b in range(R):
                kb[b * rows:b * rows + tkv, BORDER:BORDER + C] = k[b]
                vb[BORDER:BORDER + C, b * vbs:b * vbs + tkv] = v[b].T
                if tpad > tkv:
                    vb[BORDER:BORDER + C, b * vbs + tkv:b * vbs + tpad] = pad_values(C, tpad - tkv, b)
            kv.append((kb[:, BORDER:BORDER + C], rows, vb[BORDER:BORDER + C], vbs, tkv))
            kb_all += [kb, vb]
        return kv, kb_all

    if plants:
        q = G.reference("gemm", spec).want
        qh = heads_of(q, cs)
        beta = 40.0
        for _ in range(12):
            for row, sg, key in plants:
                ks[sg][:, key] = (qh[:, :, row] * beta).reshape(R, C).half()
            kv, kvb = pack()
            got = margins(cs, Ops(spec, kv, None, plants), q)
            if min(got) >= MARGIN and all(torch.isfinite(k).all() for k in ks):
                break
            beta *= 1.25
        assert min(got) >= MARGIN, (cs.name, got)
    else:
        kv, kvb = pack()
    return Ops(spec, kv, bufs + kvb, plants)


def pad_values(C, n, b, sign=1.0):
    """+-PAD_V in a checkerboard over (channel, pad column), shifted by the image index; `sign = -1` flips every one of them."""
    return (sign * PAD_V * (1 - 2 * ((torch.arange(C)[:, None] + torch.arange(n)[None, :] + b) % 2))).half()


# ---- the reference ----------------------------------------------------------------------------------------------------------------------
def _scaled(x, cs):
    return r16(x * cs.out_scale) if cs.out_scale != 1.0 else x


def reference(cs, ops=None, rounding=True):
    ops = operands(cs) if ops is None else ops
    gr = G.reference("gemm", ops.spec)          # the q projection alone: a, w, bias, ln_in
    if rounding:
        q, dq = gr.want, torch.maximum(gr.hi - gr.want, gr.want - gr.lo)
    else:
        q, dq = gr.p, torch.zeros_like(gr.p)
    qh, dqh = heads_of(q, cs), heads_of(dq, cs)
    shape = (cs.R, cs.heads, cs.Tq, D)
    value, lo_v, hi_v, mag = (torch.zeros(shape, dtype=torch.float64) for _ in range(4))
    for Kh, Vh, tkv in _kv_heads(cs, ops.kv):
        KT = Kh.transpose(-1, -2)
        s = qh @ KT
        p = torch.exp2(s - s.max(-1, keepdim=True).values)
        tot = p.sum(-1, keepdim=True)
        P = p / tot
        if not rounding:
            value += P @ Vh
            continue
        rest = (tot - p) / tot
        S = ((qh.abs() + dqh) @ KT.abs()).max(-1, keepdim=True).values
        ds = (D + KS + 2) * U * S
        Dq = torch.minimum((dqh @ KT.abs()).max(-1, keepdim=True).values,
                           (dqh @ (Kh - Kh[:, :, :1]).abs().transpose(-1, -2)).max(-1, keepdim=True).values)
        f = torch.exp2(2 * (Dq + ds))
        e1 = 2 * E_EXP + E_RCP + (tkv + 1) * U
        Pl = r16(P / (P + rest * f) * (1 - e1))
        Ph = r16((P / (P + rest / f)).clamp(max=1.0) * (1 + e1))
        Vp, Vn = Vh.clamp(min=0), (-Vh).clamp(min=0)
        value += r16(P) @ Vh
        lo_v += Pl @ Vp - Ph @ Vn
        hi_v += Ph @ Vp - Pl @ Vn
        mag += Ph @ Vh.abs()
    if not rounding:
        v = to_o_layout(value)
        return Ref(v, v, v, torch.zeros_like(v), v, torch.zeros_like(v), q, dq)
    acc = (sum(cs.tk) + 5) * U * mag
    lo_v, hi_v = lo_v - acc, hi_v + acc
    want, lo, hi = (to_o_layout(_scaled(r16(x), cs)) for x in (value, lo_v, hi_v))
    shift = to_o_layout(torch.maximum(hi_v - value, value - lo_v))
    return Ref(want, lo, hi, torch.maximum(hi - want, want - lo), to_o_layout(value), shift, q, dq)


def outside(got, ref):
    """(number of elements of `got` outside [lo, hi] or not finite, the largest |got - want| / bound: inf where the bound is 0
    and the error is not)."""
    got = got.double()
    bad = ~((got >= ref.lo) & (got <= ref.hi))          # NaN compares false: counted
    err = (got - ref.want).abs()
    err = torch.where(torch.isfinite(got), err, torch.full_like(err, float("inf")))
    ratio = torch.where(err > 0, err / ref.bound, torch.zeros_like(err))
    return int(bad.sum()), float(ratio.max())


def worst(got, ref, cs):
    """The worst element as (image, query, head, d, got, want, lo, hi)."""
    g = got.double()
    ex = torch.maximum(g - ref.hi, ref.lo - g)
    ex = torch.where(torch.isfinite(g), ex, torch.full_like(ex, float("inf")))
    i = int(ex.argmax())
    r, col = divmod(i, ref.want.shape[1])
    return dict(image=r // cs.Tq, query=r % cs.Tq, head=col // D, d=col % D, got=float(g.reshape(-1)[i]),
                want=float(ref.want.reshape(-1)[i]), lo=float(ref.lo.reshape(-1)[i]), hi=float(ref.hi.reshape(-1)[i]))


# ---- the fp32 stand-in ------------------------------------------------------------------------------------------------------------------
MUTANTS = ("mask_le", "ip_concat", "joint_softmax", "shared_max", "image0", "head_swap", "p_unrounded", "vclamp_off", "late_norm")


def q_standin(cs, ops):
    """The q tile in fp32 with the kernel's rounding: (M, C) float32 of fp16 values."""
    s = ops.spec
    if s.get("ln_in") is not None:
        return F.ln_in_standin(s).float()
    v = s["a"].float() @ s["w"].float().T
    if s.get("bias") is not None:
        v = v + s["bias"].float()[None, :]
    return v.half().float()


def images(cs, ops, mut=None):
    """The staged K image (R, H, 144, 64) and V^T image (R, H, 64, 144) in fp32, gathered from the views as the two `glds16`
    loops address them: K row r < 80 is text key min(r, Tkv - 1), row 80 + r IP key min(r, Tkv - 1); V^T chunk c of 8 key columns
    is chunk min(c, roundup8(Tkv) / 8 - 1) of the image's window."""
    Ks, Vs = [], []
    for (kview, rows, vt, vbs, tkv), width in zip(ops.kv, (KROWS_TEXT, KROWS_IP)):
        key = torch.arange(width).clamp(max=tkv - 1)
        vch = (tkv + 7) // 8
        c = torch.arange(width // 8).clamp(max=vch if mut == "vclamp_off" else vch - 1)
        col = (c[:, None] * 8 + torch.arange(8)[None, :]).reshape(-1)
        kb, vb = [], []
        for b in range(cs.R):
            bb = 0 if mut == "image0" else b
            kb.append(kview[bb * rows + key].reshape(width, cs.heads, D).permute(1, 0, 2))
            vb.append(vt[:, bb * vbs + col].reshape(cs.heads, D, width))
        Ks.append(torch.stack(kb))
        Vs.append(torch.stack(vb))
    Kimg, Vimg = torch.cat(Ks, 2).float(), torch.cat(Vs, 3).float()
    if mut == "head_swap":
        sw = torch.arange(cs.heads) ^ 1
        Kimg, Vimg = Kimg[:, sw], Vimg[:, sw]
    if mut == "ip_concat":          # IP key j taken from image row / column Tkv_text + j
        idx = torch.cat([torch.arange(KROWS_TEXT), (cs.tk[0] + torch.arange(KROWS_IP)).clamp(max=KROWS_TEXT + KROWS_IP - 1)])
        Kimg, Vimg = Kimg[:, :, idx], Vimg[..., idx]
    return Kimg, Vimg


def standin(cs, ops=None, mut=None):
    """The launch of `cs` by the fp32 stand-in; the O view's layout, float64 of the stored fp16 values.  Mutants: mask_le (the
    mask accepts key <= Tkv), ip_concat (IP keys taken from column Tkv_text, not 80), joint_softmax (one softmax over all keys),
    shared_max (one maximum for both segments, separate sums), image0 (every tile reads image 0's K / V^T), head_swap (the two
    heads of a tile swapped), p_unrounded (P stays fp32), vclamp_off (the V^T chunk clamp is roundup8(Tkv) / 8, one chunk past
    the window), late_norm (P unnormalised; 1 / sum multiplies P V of the text segment only)."""
    ops = operands(cs) if ops is None else ops
    qf = heads_of(q_standin(cs, ops), cs)
    Kimg, Vimg = images(cs, ops, mut)
    t0, t1 = cs.tk
    col = torch.arange(KROWS_TEXT + KROWS_IP)
    seg1 = col >= KROWS_TEXT
    key = torch.where(seg1, col - KROWS_TEXT, col)
    lim = torch.where(seg1, torch.full_like(col, t1), torch.full_like(col, t0))
    ok = key <= lim if mut == "mask_le" else key < lim
    ninf = -float("inf")
    s = (qf @ Kimg.transpose(-1, -2)).masked_fill(~ok, ninf)
    s0, s1 = s[..., :KROWS_TEXT], s[..., KROWS_TEXT:]
    mx0, mx1 = s0.max(-1, keepdim=True).values, s1.max(-1, keepdim=True).values
    if mut in ("shared_max", "joint_softmax"):
        mx0 = mx1 = torch.maximum(mx0, mx1)
    p0, p1 = torch.exp2(s0 - mx0), torch.exp2(s1 - mx1)
    sm0, sm1 = p0.sum(-1, keepdim=True), p1.sum(-1, keepdim=True)
    if mut == "joint_softmax":
        sm0 = sm1 = sm0 + sm1
    r0, r1 = 1.0 / sm0, 1.0 / sm1
    V0, V1 = Vimg[..., :KROWS_TEXT].transpose(-1, -2), Vimg[..., KROWS_TEXT:].transpose(-1, -2)
    if mut == "late_norm":
        o = (p0.half().float() @ V0) * r0 + p1.half().float() @ V1
    else:
        pf = torch.cat([p0 * r0, p1 * r1], -1)
        if mut != "p_unrounded":
            pf = pf.half().float()
        o = pf @ torch.cat([V0, V1], -2)
    o16 = o.half()
    if cs.out_scale != 1.0:
        o16 = (o16.float() * cs.out_scale).half()
    return to_o_layout(o16.double())


# ---- the launches of tests/test_xattn_every_case_gpu.py -----------------------------------------------------------------------------------
TK_PAIRS = ((1, 1), (80, 64), (80, 1), (1, 64), (7, 9), (8, 8), (9, 7), (16, 17), (17, 16), (65, 57), (73, 63), (79, 4))


def _cases():
    out = [
        # one workgroup; a single K tile, shorter than the 3-stage ring
        case("wg1.k64.t77_16", 1, 64, 2, 64, (77, 16)),
        case("k128.t1_1", 2, 64, 2, 128, (1, 1)),
        case("k192.t80_64.fold1", 3, 64, 2, 192, (80, 64), fold=1),                       # one tile per image, three images
        case("k320.t80_1.fold4.plant", 2, 128, 2, 320, (80, 1), fold=4, regime="plant"),  # two tiles per image, five K tiles
        case("k128.t1_64.nobias.h4", 2, 64, 4, 128, (1, 64), bias=False),
        case("k64.t7_9.big", 2, 64, 2, 64, (7, 9), regime="big"),
        case("k64.t8_8.equal", 1, 128, 2, 64, (8, 8), regime="equal"),
        case("k128.t9_7.plant", 2, 64, 2, 128, (9, 7), regime="plant"),
        case("k64.t16_17.h6", 1, 64, 6, 64, (16, 17)),
        case("k64.t17_16.big", 2, 64, 2, 64, (17, 16), regime="big"),
        case("k64.t65_57.equal", 2, 64, 2, 64, (65, 57), regime="equal"),
        case("k128.t73_63.fold4.plant.h4", 3, 64, 4, 128, (73, 63), fold=4, regime="plant"),
        case("k192.t79_4.scale", 2, 128, 2, 192, (79, 4), out_scale=0.5),
        case("k128.t77_64.fold1.nobias.equal", 2, 64, 2, 128, (77, 64), fold=1, bias=False, regime="equal"),
    ]
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    for c in out:
        assert c.R * c.Tq <= 256 and c.heads * D <= 384 and c.K <= 320 and c.Tq % 64 == 0 and c.heads % 2 == 0 and c.K % 64 == 0
        assert 1 <= c.tk[0] <= 80 and 1 <= c.tk[1] <= 64 and (not c.fold or c.K % c.fold == 0)
    return {c.name: c for c in out}


CASES = _cases()

# the case at which tests/test_xattn_ref_cpu.py shows each mutant outside the interval
CAUGHT_AT = {
    "mask_le": "k64.t7_9.big",                         # key Tkv: the last key again, with a +-1000 pad column as its V
    "ip_concat": "wg1.k64.t77_16",                     # Tkv_text < 80
    "joint_softmax": "wg1.k64.t77_16",
    "shared_max": "k64.t17_16.big",                    # the segments' maxima lie > 150 log2 units apart in some rows
    "image0": "k192.t80_64.fold1",                     # R = 3
    "head_swap": "k64.t16_17.h6",
    "p_unrounded": "k128.t77_64.fold1.nobias.equal",   # P = 1 / 77 and 1 / 64: round16(1 / 77) is 1.4e-4 below it
    "vclamp_off": "k128.t9_7.plant",                   # the chunk past the window holds NaN (a neighbour's keys in a dense layout)
    "late_norm": "k64.t65_57.equal",                   # the IP sum is 57, not 1
}


LOG_HEADER = "# case | R x Tq x heads, K, (Tkv text, Tkv ip) | elements | != want | kernel worst err/bound | stand-in worst err/bound | kernel wall ms (launch + sync, not a benchmark)"
