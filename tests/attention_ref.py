"""fp64 restatement of one `ops.attention` launch (head dim 64 / 80 / 104), with a per-element bound derived from the number
formats, the fp32 stand-ins of the two kernels, and the seeded launches of tests/test_attention_every_build_gpu.py.  Plain helper
for that file and for tests/test_attention_ref_cpu.py; no GPU use.

`reference(case, ops)` returns a `Ref` in the layout of the O view, (batch * Tq, heads * D) float64: `want`, `lo`, `hi`,
`bound = max(hi - want, want - lo)`, and `value`, `shift` (before the output rounding).  `reference(..., rounding=False)` drops
every rounding point: plain softmax(q k^T scale) v, summed over the segments.

Rounding points (the ones csrc/attention.hip and csrc/attention_hd.hip document, no others)
  d64      q' = fp16(fp32(q) * c), c = fp32(fp32(scale) * fp32(log2 e)) (`attn_geo`); q' = q when `q_prescaled`.  Scores q' . k
           and the base-2 softmax in fp64 from there.
  80, 104  Q as given; score * c in the softmax, c as above and c = 1 when `q_prescaled` (`iir_attention_f16`).
  two segments: d64 holds the first segment's normalised result as fp16 (`ohold`) and adds it to the second; the hd kernel adds
           the two in fp32 (no rounding).
  output   fp16, then (o_fp8) that fp16 value to E4M3 as `iir_fp8x4` does (`to_e4m3` of the GEMM reference).
  identity rows (`ident_from`): O = V, exactly; bound 0.

The bound.  Per segment, let P be the normalised fp64 probabilities, A = P @ |V|, A_a the part of A that comes from keys in the
first 32 of their 64-key tile (d64: the half whose P waits in fp16 while the second half is tested), Vis = (visible keys) @ |V|,
Vis_a likewise, S = max over the row's visible keys of sum_d |q'_d k_d| (times c at 80 / 104), KS = ceil(D / 16) the MFMA chain
of a score and n the number of online-softmax steps of the segment (d64: 2 per tile; hd: 1 per tile).  The kernel's normalised
value, before any rounding of the output, differs from the reference's by at most

  shift = u_P * (A + 2 A_a)                                  P is rounded to fp16 (u_P = 2^-11, relative, at whatever maximum the
                                                             kernel holds).  d64: when half b raises the maximum, half a's packed
                                                             P is multiplied by ah = fp16(2^-delta) in fp16 -- two more roundings
                                                             for those keys (rows that ride along with 0 < delta have them too).
                                                             A_a = 0 at 80 / 104.
        + (2^(2 ds) - 1) * A                                 a score off by ds (log2 units) moves numerator and denominator by
                                                             2^(+-ds) each.  ds = (D + KS + 2 n) * 2^-24 * S: D for the fp32
                                                             accumulation of the D products in any order, KS for the roundings of
                                                             the chain with -m riding in the C operand (|m| <= S), 2 per step for
                                                             m + delta and the `a - delta` / `c1 - delta` / `fma(s, c, -m)`
                                                             updates, whose roundings are of magnitude <= S and shift every later
                                                             score of the row.
        + 2 * E_EXP * A                                      v_exp_f32 on numerator and denominator.  The ISA text in the guides
                                                             gives no error for it: E_EXP = 2^-23 (1 ulp of fp32) is assumed;
                                                             NOBODY MEASURED IT.  (A rescale multiplies O and l by the same
                                                             alpha, so alpha's own error cancels.)
        + (2 Tkv + 2 n + 4) * 2^-24 * A                      fp32 accumulation of l and of P.V over Tkv terms, one multiply of
                                                             both per step, and the reciprocal / normalisation / segment add.
        + 2^-25 * Vis + (2^THR + 1) * 2^-25 * Vis_a          underflow, absolute.  The kernel's maximum m never exceeds the true
                                                             running maximum (it is raised by the row's own excess), so l >= 1
                                                             and a P that is subnormal or 0 in fp16 is off by <= 2^-25 (half
                                                             the subnormal step) per key, smaller after later rescales.  d64,
                                                             half-a keys: the product pa * ah is rounded again (2^-25), and
                                                             ah itself is subnormal for delta > 14 and 0 for delta > 25:
                                                             |ah - 2^-delta| <= 2^-25 times pa <= 2^THR (the lag of the lazy
                                                             maximum).  Order Tkv * 2^-24 * max|V|, as expected.

`lo` / `hi` are the images of value -+ shift under the roundings above (monotone), not a closed form u |want| + shift: as the
GEMM reference found, a correct kernel breaks the closed form at rounding ties.  With two segments (d64) the interval of
segment 1 goes through its fp16 rounding before the add.  Nothing here comes from a kernel's output; no term is measured.

Room left on one MI355X (the kernels' outputs over every case of the GPU file) is in profiles/attention_every_build.log and
quoted per build in DESIGN.md.
"""
import collections
import functools

import numpy as np
import torch
import torch.nn.functional as F

from gemm_conv_ref import to_e4m3

KT = 64
THR = 5.0                       # csrc/attention.hip
LOG2E32 = np.float32(1.4426950408889634)
U_P = 2.0 ** -11
E_EXP = 2.0 ** -23              # assumed: 1 ulp of fp32 (not in the ISA text at hand, not measured)
BORDER = 8
SENTINEL = 7.0
SENTINEL8 = 0x55
PAD_V = 1000.0

Case = collections.namedtuple("Case", "name D B heads Tq tkvs kv_rows scale causal qpre ident_from o_fp8 sig plants")
Ops = collections.namedtuple("Ops", "q kv bufs")          # q: view; kv: [(k view, rows, vt view, vbs, Tkv)]; bufs: whole buffers
Ref = collections.namedtuple("Ref", "want lo hi bound value shift")


def case(name, D=64, B=2, heads=2, Tq=128, tkvs=(64,), kv_rows=None, scale=None, causal=False, qpre=False, ident_from=0,
         o_fp8=False, sig=1.0, plants=()):
    return Case(name, D, B, heads, Tq, tuple(tkvs), tuple(kv_rows or tkvs), float(D ** -0.5 if scale is None else scale), causal, qpre,
                ident_from, o_fp8, sig, tuple(plants))


def c_of(cs):
    """`attn_geo`: g.c = a->scale * 1.4426950408889634f, in fp32."""
    return np.float32(np.float32(cs.scale) * LOG2E32)


def roundup8(n):
    return (n + 7) // 8 * 8


# ---- which kernel runs ----------------------------------------------------------------------------------------------------------------
def build_of(cs):
    """The selection rule of `launch_attn` (csrc/attention.hip, the `if (!g.causal && total_tiles <= 4)` ladder) and of
    `iir_attention_f16` (csrc/attention_hd.hip) restated; n_attn as `attn_geo` (csrc/attn_geo.h) forms it."""
    if cs.D != 64:
        return f"hd{cs.D}"
    total = sum((t + KT - 1) // KT for t in cs.tkvs)
    n_attn = cs.heads * (cs.ident_from or cs.B) * ((cs.Tq + 127) // 128)
    b = "pre" if (not cs.causal and total <= 4) else ("ring2" if n_attn <= 512 else "ring3")
    return b + (".ident" if cs.ident_from else "")


def n_attending(cs):
    return cs.heads * (cs.ident_from or cs.B) * ((cs.Tq + 127) // 128)


def tiles_of(cs, Tkv):
    """[(tile, FIRST, MASKED)] of one segment: the three loops at the end of `attn_kernel2`'s segment body."""
    nt = (Tkv + KT - 1) // KT
    ragged = Tkv % KT != 0
    out = [(0, True, bool(cs.causal or (ragged and nt == 1)))]
    if not cs.causal:
        out += [(t, False, False) for t in range(1, nt - 1 if ragged else nt)]
    first_masked = 1 if cs.causal else (nt - 1 if (ragged and nt > 1) else nt)
    return out + [(t, False, True) for t in range(first_masked, nt)]


# ---- operands ---------------------------------------------------------------------------------------------------------------------------
def _gen(name):
    return torch.Generator().manual_seed(int.from_bytes(name.encode(), "little") % (2 ** 31 - 1))


def _scores64(cs, q, k):
    """fp64 scores in log2 units of (Tq, D) x (Tkv, D) fp16 operands as the kernel of `cs` forms them."""
    c = float(c_of(cs))
    if cs.D == 64:
        qq = q.double() if cs.qpre else (q.float() * c).half().double()
        return qq @ k.double().T
    return (q.double() @ k.double().T) * (1.0 if cs.qpre else c)


def _plant(cs, q, ks):
    """Plant keys.  A plant (row, seg, key, kind) sets k[seg][b, key, head] = beta * (the row's q as the kernel scores it), so the
    row's score at `key` rises above every earlier key of the segment: kind "p" (beta = 8 / sig^2, ~90 log2 units; grown until
    the rise is >= 30), "p2" (twice that: a second rise in the same row), "huge" (rise >= 160: alpha = 0 and ah = 0), "mid" (beta
    bisected until the rise lies in [15, 18], so the lazy maximum's delta lies in (14, 24]: ah is an fp16 subnormal).  Every
    margin is checked in fp64 on the fp16 values after rounding."""
    D = cs.D
    for row, sg, key, kind in sorted(cs.plants, key=lambda p: (p[1], p[2])):
        assert key < cs.tkvs[sg] and row < cs.Tq and (not cs.causal or key <= row)
        for b in range(cs.B):
            for h in range(cs.heads):
                sl = slice(h * D, (h + 1) * D)
                qd = q[b, row, sl].double()
                if cs.qpre:
                    qd = qd / float(c_of(cs))
                prev = _scores64(cs, q[b, row:row + 1, sl], ks[sg][b, :max(key, 1), sl])[0]
                prev_max = float(prev.max()) if key else -1e30

                def rise(beta):
                    kk = (qd * beta).half()
                    return float(_scores64(cs, q[b, row:row + 1, sl], kk[None])[0, 0]) - prev_max, kk
                base = 8.0 / cs.sig ** 2
                if kind == "mid":
                    lo, hi = 0.0, base
                    for _ in range(40):
                        mid = 0.5 * (lo + hi)
                        r, kk = rise(mid)
                        if 15.5 <= r <= 17.5:
                            break
                        lo, hi = (mid, hi) if r < 16.5 else (lo, mid)
                    assert 15.0 <= r <= 18.0, (cs.name, r)
                else:
                    beta, need = {"p": base, "p2": 2 * base, "huge": 3 * base}[kind], (160.0 if kind == "huge" else 30.0)
                    r, kk = rise(beta)
                    while r < need and beta < 64 * base:          # a short q or a high earlier maximum: a longer key
                        beta *= 1.25
                        r, kk = rise(beta)
                    assert r >= need and torch.isfinite(kk).all(), (cs.name, kind, r)
                ks[sg][b, key, sl] = kk


@functools.lru_cache(maxsize=None)
def operands(cs):
    """The launch of `cs` as the GPU file issues it, on the CPU: Q / K column slices of buffers with NaN beside them; NaN in the K
    rows between Tkv and `kv_rows` of every batch; V^T a row slice with NaN rows beside the heads and NaN columns outside its
    window, +-PAD_V on [Tkv, roundup8(Tkv)).  (The O buffer is made by the GPU file: `out_buffer`.)"""
    g = _gen(cs.name)
    B, Tq, C, D = cs.B, cs.Tq, cs.heads * cs.D, cs.D
    q = (torch.randn(B, Tq, C, generator=g) * cs.sig).half()
    if cs.qpre:
        q = (q.float() * float(c_of(cs))).half()
    ks = [(torch.randn(B, t, C, generator=g) * cs.sig).half() for t in cs.tkvs]
    vs = [torch.randn(B, t, C, generator=g).half() for t in cs.tkvs]
    if cs.ident_from:
        assert len(cs.tkvs) == 1 and cs.tkvs[0] == Tq
    _plant(cs, q, ks)
    nan = float("nan")
    qb = torch.full((B * Tq, C + 2 * BORDER), nan, dtype=torch.half)
    qb[:, BORDER:BORDER + C] = q.reshape(-1, C)
    kv, bufs = [], [qb]
    for k, v, tkv, rows in zip(ks, vs, cs.tkvs, cs.kv_rows):
        vbs, tpad = roundup8(rows), roundup8(tkv)
        kb = torch.full((B * rows, C + 2 * BORDER), nan, dtype=torch.half)
        vb = torch.full((C + 2 * BORDER, B * vbs + 64), nan, dtype=torch.half)
        for b in range(B):
            kb[b * rows:b * rows + tkv, BORDER:BORDER + C] = k[b]
            vb[BORDER:BORDER + C, b * vbs:b * vbs + tkv] = v[b].T
            if tpad > tkv:
                pad = PAD_V * (1 - 2 * ((torch.arange(C)[:, None] + torch.arange(tpad - tkv)[None, :] + b) % 2)).half()
                vb[BORDER:BORDER + C, b * vbs + tkv:b * vbs + tpad] = pad
        kv.append((kb[:, BORDER:BORDER + C], rows, vb[BORDER:BORDER + C], vbs, tkv))
        bufs += [kb, vb]
    return Ops(qb[:, BORDER:BORDER + C], kv, bufs)


def unpack(cs, ops):
    """q (B, H, Tq, D) and per segment K (B, H, Tkv, D), Vp (B, H, roundup8(Tkv), D) [pad columns included], read from the views."""
    B, H, D, Tq = cs.B, cs.heads, cs.D, cs.Tq
    q = ops.q.reshape(B, Tq, H, D).permute(0, 2, 1, 3)
    segs = []
    for kview, rows, vt, vbs, tkv in ops.kv:
        K = kview.reshape(B, rows, H, D)[:, :tkv].permute(0, 2, 1, 3)
        tpad = roundup8(tkv)
        Vp = torch.stack([vt[:, b * vbs:b * vbs + tpad].reshape(H, D, tpad).permute(0, 2, 1) for b in range(B)])
        segs.append((K, Vp, tkv))
    return q, segs


def to_o_layout(x):
    """(B, H, Tq, D) -> the O view's (B * Tq, H * D)."""
    B, H, T, D = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * T, H * D)


def r16(x):
    return torch.from_numpy(x.numpy().astype(np.float16).astype(np.float64))


def _visible(cs, Tq, Tkv):
    vis = torch.ones(Tq, Tkv, dtype=torch.bool)
    if cs.causal:
        vis &= torch.arange(Tkv)[None, :] <= torch.arange(Tq)[:, None]
    return vis


# ---- the reference ----------------------------------------------------------------------------------------------------------------------
def reference(cs, ops=None, rounding=True):
    ops = operands(cs) if ops is None else ops
    q, segs = unpack(cs, ops)
    B, H, D, Tq = cs.B, cs.heads, cs.D, cs.Tq
    c = float(c_of(cs))
    d64 = D == 64
    nb = cs.ident_from or B
    vals, shifts = [], []
    for K, Vp, Tkv in segs:
        vis = _visible(cs, Tq, Tkv)
        half_a = (torch.arange(Tkv) % KT < 32).double() if d64 else torch.zeros(Tkv, dtype=torch.float64)
        n = (Tkv + KT - 1) // KT * (2 if d64 else 1)
        KS = (D + 15) // 16
        val, shift = torch.zeros(B, H, Tq, D, dtype=torch.float64), torch.zeros(B, H, Tq, D, dtype=torch.float64)
        for b in range(nb):
            qd, kd, vd = q[b].double(), K[b].double(), Vp[b, :, :Tkv].double()
            if not rounding:
                qs = qd if cs.qpre else qd * (cs.scale * 1.4426950408889634)
                kc = 1.0
            elif d64:
                qs = qd if cs.qpre else (q[b].float() * c).half().double()
                kc = 1.0
            else:
                qs, kc = qd, (1.0 if cs.qpre else c)
            s = (qs @ kd.transpose(-1, -2)) * kc
            s = s.masked_fill(~vis, -float("inf"))
            p = torch.exp2(s - s.max(-1, keepdim=True).values)
            P = p / p.sum(-1, keepdim=True)
            val[b] = P @ vd
            if rounding:
                av = vd.abs()
                A, A_a = P @ av, (P * half_a) @ av
                Vis, Vis_a = vis.double() @ av, (vis.double() * half_a) @ av
                S = ((qs.abs() @ kd.abs().transpose(-1, -2)) * kc).masked_fill(~vis, 0.0).max(-1, keepdim=True).values
                ds = (D + KS + 2 * n) * 2.0 ** -24 * S
                shift[b] = (U_P * (A + 2 * A_a) + (torch.exp2(2 * ds) - 1) * A + 2 * E_EXP * A + (2 * Tkv + 2 * n + 4) * 2.0 ** -24 * A
                            + 2.0 ** -25 * Vis + (2.0 ** THR + 1) * 2.0 ** -25 * Vis_a)
        vals.append(val)
        shifts.append(shift)
    if not rounding:
        v = to_o_layout(sum(vals))
        return Ref(v, v, v, torch.zeros_like(v), v, torch.zeros_like(v))
    if len(segs) == 2 and d64:          # ohold: segment 1 through its fp16 rounding, then the add
        v1 = r16(vals[0])
        value, shift = v1 + vals[1], shifts[1]
        lo, hi = r16(vals[0] - shifts[0]) + vals[1] - shifts[1], r16(vals[0] + shifts[0]) + vals[1] + shifts[1]
    else:
        value, shift = sum(vals), sum(shifts)
        lo, hi = value - shift, value + shift
    slack = 2.0 ** -23 * value.abs()            # the fp32 add of the segments
    want, lo, hi = r16(value), r16(lo - slack), r16(hi + slack)
    if cs.o_fp8:
        want, lo, hi = to_e4m3(want), to_e4m3(lo), to_e4m3(hi)
    if cs.ident_from:
        V = segs[0][1][:, :, :Tq].double()
        for t in (want, lo, hi, value):
            t[cs.ident_from:] = V[cs.ident_from:]
        shift[cs.ident_from:] = 0
    want, lo, hi = to_o_layout(want), to_o_layout(lo), to_o_layout(hi)
    return Ref(want, lo, hi, torch.maximum(hi - want, want - lo), to_o_layout(value), to_o_layout(shift))


def compare(got, want, bound):
    """(number of elements with |got - want| > bound or a non-finite `got`, the worst err / bound: inf where bound is 0 and err not)."""
    got, want, bound = got.double(), want.double(), bound.double()
    err = (got - want).abs()
    err = torch.where(torch.isfinite(got), err, torch.full_like(err, float("inf")))
    bad = err > bound
    ratio = torch.where(err > 0, err / bound, torch.zeros_like(err))
    return int(bad.sum()), float(ratio.max())


def room(got, want, bound):
    """Largest used fraction of the bound, |got - want| / bound over the elements that have any (bound > 0): near 1 for a bound of
    one rounding step, and never small unless the bound is vacuous."""
    err = (got.double() - want).abs()
    ok = bound > 0
    return float((err[ok] / bound[ok]).max()) if ok.any() else 0.0


def worst(got, ref, cs):
    """The worst element as (batch, query, head, d, got, want, lo, hi): which (tile, half, row) to read the kernel at."""
    err = (got.double() - ref.want).abs() - ref.bound
    err = torch.where(torch.isfinite(got.double()), err, torch.full_like(err, float("inf")))
    i = int(err.argmax())
    r, col = divmod(i, ref.want.shape[1])
    return dict(batch=r // cs.Tq, query=r % cs.Tq, head=col // cs.D, d=col % cs.D, got=float(got.reshape(-1)[i]),
                want=float(ref.want.reshape(-1)[i]), lo=float(ref.lo.reshape(-1)[i]), hi=float(ref.hi.reshape(-1)[i]))


# ---- the fp32 stand-ins -----------------------------------------------------------------------------------------------------------------
MUTANTS = ("ragged_off_by_one", "causal_ge", "causal_gt1", "rise_o_only", "rise_l_only", "no_c1_fix", "no_pending_scale",
           "seg2_inherits", "k_perm", "no_log2e", "c_twice", "head_xor", "batch0_vt", "pad_col", "fp8_from_fp32")


def any32(x):
    """`__any` over a wave: 32 consecutive queries (q0 = 128 * tile + 32 * wave; the clamped rows past Tq repeat row Tq - 1)."""
    B, H, T = x.shape
    y = F.pad(x, (0, (-T) % 32)).reshape(B, H, -1, 32).any(-1, keepdim=True).expand(-1, -1, -1, 32)
    return y.reshape(B, H, -1)[..., :T]


def _hidden(cs, keys, Tq, limit, mut):
    h = (keys >= limit)[None, :].expand(Tq, -1).clone()
    if cs.causal:
        qr = torch.arange(Tq)[:, None]
        h |= (keys[None, :] >= qr) if mut == "causal_ge" else (keys[None, :] > qr + 1) if mut == "causal_gt1" else (keys[None, :] > qr)
    return h


def _mutate_operands(cs, K, Vp, Tkv, mut):
    if mut == "head_xor" and cs.heads % 2 == 0:
        K = K[:, torch.arange(cs.heads) ^ 1]
    if mut == "batch0_vt":
        Vp = Vp[:1].expand(cs.B, -1, -1, -1)
    if mut == "k_perm":
        k = torch.arange(Tkv)
        pk = (k & ~12) | ((k & 4) << 1) | ((k & 8) >> 1)
        K = K[:, :, pk.clamp(max=Tkv - 1)]
    return K, Vp


def standin(cs, ops=None, mut=None, trace=None):
    """The launch of `cs` by the fp32 stand-in of its kernel; the O view's layout, float64 of the stored fp16 / E4M3 values.  `mut`
    names one deliberate fault (MUTANTS); `trace` (a list) receives one dict per threshold test of the d64 algorithm."""
    ops = operands(cs) if ops is None else ops
    out = (_standin_d64 if cs.D == 64 else _standin_hd)(cs, ops, mut, trace)
    o16 = out.half()
    if cs.o_fp8:
        res = to_e4m3(out if mut == "fp8_from_fp32" else o16)
    else:
        res = o16.double()
    if cs.ident_from:
        res[cs.ident_from:] = unpack(cs, ops)[1][0][1][cs.ident_from:, :, :cs.Tq].double()
    return to_o_layout(res)


def _standin_d64(cs, ops, mut, trace):
    """attn_kernel2 / attn_tile in torch, vectorised over (batch, head, query): 64-key tiles as two 32-key halves, m from the first
    half, the THR test per half on any of a wave's 32 rows, delta = max(mx, 0), P packed to fp16, l from the unrounded P, the fp16
    `ah` on the pending half, the masked tiles' c1, ohold in fp16."""
    q, segs = unpack(cs, ops)
    B, H, Tq = cs.B, cs.heads, cs.Tq
    c = float(np.float32(cs.scale) if mut == "no_log2e" else c_of(cs))
    qf = q.float()
    if not cs.qpre or mut == "c_twice":
        qf = (qf * c).half().float()
    ninf = -float("inf")
    ohold = None
    m = l = None
    for sg, (K, Vp, Tkv) in enumerate(segs):
        K, Vp = _mutate_operands(cs, K, Vp, Tkv, mut)
        tpad = Vp.shape[2]
        limit = Tkv + 1 if mut == "ragged_off_by_one" else tpad if mut == "pad_col" else Tkv
        inherit = mut == "seg2_inherits" and sg == 1
        if not inherit:
            m, l = torch.zeros(B, H, Tq), torch.zeros(B, H, Tq)
        O = torch.zeros(B, H, Tq, 64)

        def rescale(delta, late):
            nonlocal m, l, O
            alpha = torch.exp2(-delta)
            if not (late and mut == "rise_o_only"):
                l = l * alpha
            if not (late and mut == "rise_l_only"):
                O = O * alpha[..., None]
            m = m + delta

        for t, FIRST, MASKED in tiles_of(cs, Tkv):
            FIRST = FIRST and not inherit
            keys = torch.arange(t * KT, (t + 1) * KT)
            Kt = K[:, :, keys.clamp(max=Tkv - 1)].float()
            Vt = Vp[:, :, torch.where(keys < tpad, keys, torch.zeros_like(keys))].float()
            hid = _hidden(cs, keys, Tq, limit, mut) if MASKED else torch.zeros(Tq, KT, dtype=torch.bool)
            sraw = qf @ Kt.transpose(-1, -2)
            base = torch.zeros(B, H, Tq) if FIRST else -m
            cmask = torch.where(hid, torch.full((), ninf), torch.zeros(()))
            ca, cb = base[..., None] + cmask[:, :32], base[..., None] + cmask[:, 32:]
            # ---- half a
            sa = sraw[..., :32] + ca
            mx = sa.max(-1).values
            if FIRST:
                m = mx
                sa, cb = sa - mx[..., None], cb - mx[..., None]
            else:
                trig = any32(mx > THR)
                delta = torch.where(trig, mx.clamp(min=0), torch.zeros(()))
                rescale(delta, True)
                sa = sa - delta[..., None]
                if not (MASKED and mut == "no_c1_fix"):
                    cb = cb - delta[..., None]
                if trace is not None:
                    trace.append(dict(seg=sg, tile=t, half="a", first=FIRST, masked=MASKED, fired=bool(trig.any()), delta=delta))
            pa32 = torch.exp2(sa)
            ls = pa32.sum(-1)
            pa = pa32.half()
            # ---- half b
            sb = sraw[..., 32:] + cb
            mxb = sb.max(-1).values
            trig = any32(mxb > THR)
            delta = torch.where(trig, mxb.clamp(min=0), torch.zeros(()))
            ah = torch.exp2(-delta).half()
            if mut != "no_pending_scale":
                pa = (pa.float() * ah.float()[..., None]).half()
            ls = ls * torch.exp2(-delta)
            rescale(delta, not FIRST)
            sb = sb - delta[..., None]
            if trace is not None:
                trace.append(dict(seg=sg, tile=t, half="b", first=FIRST, masked=MASKED, fired=bool(trig.any()), delta=delta))
            O = O + pa.float() @ Vt[:, :, :32]
            pb32 = torch.exp2(sb)
            l = l + (ls + pb32.sum(-1))
            O = O + pb32.half().float() @ Vt[:, :, 32:]
        o = O * (1.0 / l)[..., None]
        if sg + 1 < len(segs):
            ohold = o.half()
        elif ohold is not None:
            o = o + ohold.float()
    return o


def _standin_hd(cs, ops, mut, trace):
    """attn_hd_kernel: the maximum raised eagerly per 64-key tile, score * c inside the softmax, the segments added in fp32."""
    q, segs = unpack(cs, ops)
    B, H, Tq, D = cs.B, cs.heads, cs.Tq, cs.D
    c = float(np.float32(cs.scale) if mut == "no_log2e" else c_of(cs))
    if cs.qpre and mut != "c_twice":
        c = 1.0
    qf = q.float()
    ninf = -float("inf")
    out = torch.zeros(B, H, Tq, D)
    m = l = None
    for sg, (K, Vp, Tkv) in enumerate(segs):
        K, Vp = _mutate_operands(cs, K, Vp, Tkv, mut)
        tpad = Vp.shape[2]
        limit = Tkv + 1 if mut == "ragged_off_by_one" else tpad if mut == "pad_col" else Tkv
        if not (mut == "seg2_inherits" and sg == 1):
            m, l = torch.full((B, H, Tq), ninf), torch.zeros(B, H, Tq)
        O = torch.zeros(B, H, Tq, D)
        for t in range((Tkv + KT - 1) // KT):
            keys = torch.arange(t * KT, (t + 1) * KT)
            Kt = K[:, :, keys.clamp(max=Tkv - 1)].float()
            Vt = Vp[:, :, torch.where(keys < tpad, keys, torch.zeros_like(keys))].float()
            s = (qf @ Kt.transpose(-1, -2)).masked_fill(_hidden(cs, keys, Tq, limit, mut), ninf)
            m_new = torch.maximum(m, s.max(-1).values * c)
            alpha = torch.exp2(m - m_new)
            if mut != "rise_o_only":
                l = l * alpha
            if mut != "rise_l_only":
                O = O * alpha[..., None]
            m = m_new
            p = torch.exp2(s * c - m[..., None])
            l = l + p.sum(-1)
            O = O + p.half().float() @ Vt
        out = out + O * (1.0 / l)[..., None]
    return out


# ---- the launches of tests/test_attention_every_build_gpu.py ----------------------------------------------------------------------------
PEAK = 8 ** 0.5          # q, k ~ N(0, sqrt 8) per element: score std 8, peaked rows (tests/test_vae_flash_attention_gpu.py)


def _placements(Tkv):
    """One planted rise per placement, in rows of different waves (the other 31 rows of each wave ride along): FIRST tile half b;
    steady tile half a; steady tile half b; both halves of one steady tile; the masked last tile's half a and half b.  Needs
    Tkv % 64 > 32 and >= 4 tiles."""
    last = Tkv // KT * KT
    assert Tkv % KT > 32 and last >= 192
    return ((1, 0, 40, "p"), (33, 0, 70, "p"), (65, 0, 100, "p"), (97, 0, 130, "p"), (97, 0, 170, "p2"),
            (5, 0, last + 3, "p"), (37, 0, last + 35, "p"))


def _cases():
    out = []
    add = lambda *a, **k: out.append(case(*a, **k))
    tqs = (1, 33, 128, 129)
    # ---- d64, every tile staged at entry
    for i, T in enumerate((1, 7, 8, 9, 63, 64, 65, 200, 256)):
        add(f"pre.t{T}", Tq=tqs[i % 4], tkvs=[T], sig=PEAK if i % 2 else 1.0)
    add("pre.place.n1", Tq=129, tkvs=[250], plants=_placements(250))
    add("pre.place.n8", Tq=129, tkvs=[250], plants=_placements(250), sig=PEAK)
    add("pre.2seg.77.64", Tq=129, tkvs=[77, 64])
    add("pre.2seg.77.64.n8", Tq=129, tkvs=[77, 64], sig=PEAK)
    add("pre.2seg.1.130", Tq=33, tkvs=[1, 130])
    add("pre.qpre", Tq=129, tkvs=[77, 64], qpre=True)
    add("pre.o_fp8", Tq=128, tkvs=[200], o_fp8=True)
    add("pre.o_fp8.2seg.n8", Tq=33, tkvs=[77, 64], o_fp8=True, sig=PEAK)
    add("pre.scale", Tq=33, tkvs=[65], scale=0.2)
    add("pre.huge", Tq=129, tkvs=[200], plants=((1, 0, 100, "huge"), (33, 0, 130, "huge"), (65, 0, 40, "huge")))
    add("pre.mid", Tq=129, tkvs=[200], plants=((1, 0, 100, "mid"), (33, 0, 130, "mid"), (65, 0, 40, "mid")))
    # ---- d64, ring for 2 waves per SIMD
    add("ring2.t257", Tq=33, tkvs=[257])
    add("ring2.place.n1", Tq=129, tkvs=[300], plants=_placements(300))
    add("ring2.place.n8", Tq=129, tkvs=[300], plants=_placements(300), sig=PEAK)
    add("ring2.t320", Tq=128, tkvs=[320], sig=PEAK)
    add("ring2.2seg.300.77", Tq=129, tkvs=[300, 77])
    add("ring2.2seg.64.257.n8", Tq=33, tkvs=[64, 257], sig=PEAK)
    add("ring2.causal77", Tq=77, tkvs=[77], kv_rows=[80], causal=True)
    add("ring2.causal80over77", Tq=80, tkvs=[77], kv_rows=[80], causal=True, sig=PEAK)
    add("ring2.causal200", Tq=200, tkvs=[200], causal=True, plants=((150, 0, 40, "p"), (199, 0, 140, "p"), (199, 0, 170, "p2"), (180, 0, 70, "p")))
    add("ring2.causal200.n8", Tq=200, tkvs=[200], causal=True, sig=PEAK)
    add("ring2.causal50x136", Tq=50, tkvs=[136], causal=True)
    add("ring2.causal.qpre", Tq=77, tkvs=[77], causal=True, qpre=True)
    add("ring2.huge", Tq=33, tkvs=[300], plants=((1, 0, 290, "huge"), (2, 0, 260, "huge")))
    # ---- d64, ring for 3 waves per SIMD: 19 x 27 pairs x 1 query tile = 513 attending workgroups
    add("ring3.place.n8", B=19, heads=27, Tq=100, tkvs=[360], plants=_placements(360), sig=PEAK)
    add("ring3.t330", B=19, heads=27, Tq=100, tkvs=[330])
    add("ring3.causal77", B=19, heads=27, Tq=77, tkvs=[77], kv_rows=[80], causal=True)
    add("ring3.2seg", B=19, heads=27, Tq=40, tkvs=[300, 77])
    # ---- grids of 1, 7, 8, 9 and 520 attending workgroups (513: above) through attn_lin
    for n, (B, h) in {1: (1, 1), 7: (1, 7), 8: (2, 4), 9: (3, 3)}.items():
        add(f"grid{n}", B=B, heads=h, Tq=40, tkvs=[65], sig=PEAK if n % 2 else 1.0)
    add("grid520", B=20, heads=26, Tq=40, tkvs=[257])
    add("grid9.hd80", D=80, B=3, heads=3, Tq=40, tkvs=[65])
    # ---- d64 identity form
    for T in (5, 13, 192, 200):
        add(f"ident.pre.t{T}", B=3, Tq=T, tkvs=[T], ident_from=2, sig=PEAK if T == 200 else 1.0)
    add("ident.ring2.t321", B=3, Tq=321, tkvs=[321], ident_from=2)
    add("ident.ring3.t257", B=10, heads=19, Tq=257, tkvs=[257], ident_from=9)
    # ---- head dims 80 / 104
    for D in (80, 104):
        for sig, tag in ((1.0, "n1"), (PEAK, "n8")):
            add(f"hd{D}.ragged.{tag}", D=D, Tq=33, tkvs=[50], sig=sig)
            add(f"hd{D}.late.{tag}", D=D, Tq=129, tkvs=[200], sig=sig, plants=((1, 0, 190, "p"), (33, 0, 70, "p"), (33, 0, 130, "p2")))
            add(f"hd{D}.causal.{tag}", D=D, Tq=77, tkvs=[77], causal=True, sig=sig)
            add(f"hd{D}.2seg.{tag}", D=D, Tq=100, tkvs=[77, 130], sig=sig)
            add(f"hd{D}.qpre.{tag}", D=D, Tq=129, tkvs=[200], qpre=True, sig=sig)
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return {c.name: c for c in out}


CASES = _cases()


def plain_of(cs):
    """The identity case's attending rows as a launch of their own: same buffers, batch = ident_from."""
    return cs._replace(B=cs.ident_from, ident_from=0)
