"""LQ fidelity guidance restated for the tests, independent of the product's arithmetic (nothing here imports instantir_amd):

  lowpass / correct      fp64: LP, a separable Gaussian (radius ceil(3 sigma)) whose out-of-image taps are dropped and whose axes
                         are renormalised by the in-image taps' sum; delta = w LP(z - x0), x0' = x0 + delta, prev' = prev + c delta
  lowpass32 / correct32  the same with the kernel's fp32 rounding points (fp32 taps, fmaf in tap order, fp32 norm, one division
                         per axis, no contraction in the pointwise half): what the derived bound is first checked against
  bound                  the derived element-wise tolerance of a launch
  fidelity               the method as a `guide(rows, i, t, x, coef)` hook of oracle.pipeline.denoise / loop_ref.sigma_denoise,
                         wrapped around any other hook of loop_ref (cfg_guide, apg, perturbed)
"""
import math

import numpy as np
import torch


def radius(sigma):
    return int(math.ceil(3.0 * float(sigma)))


def taps64(sigma):
    """2 r + 1 Gaussian taps, sum 1, fp64 (numpy); empty for sigma = 0"""
    r = radius(sigma)
    if r == 0:
        return np.zeros(0)
    g = np.exp(-0.5 * ((np.arange(2 * r + 1, dtype=np.float64) - r) / float(sigma)) ** 2)
    return g / g.sum()


def axis_matrix(n, sigma):
    """(n, n) fp64: row i holds the taps that fall inside [0, n) around i, divided by their sum"""
    r, g = radius(sigma), taps64(sigma)
    M = np.zeros((n, n))
    for i in range(n):
        for j in range(2 * r + 1):
            q = i + j - r
            if 0 <= q < n:
                M[i, q] = g[j]
        M[i] /= M[i].sum()
    return torch.from_numpy(M)


def lowpass(d, sigma):
    """LP over the last two axes of an fp64 tensor; the identity for sigma = 0"""
    if radius(sigma) == 0:
        return d.double()
    H, W = d.shape[-2:]
    return axis_matrix(H, sigma) @ d.double() @ axis_matrix(W, sigma).T


def correct(x0, z, prev, w, c, sigma):
    """fp64 -> (x0', prev', delta)"""
    delta = float(w) * lowpass(z.double() - x0.double(), sigma)
    return x0.double() + delta, prev.double() + float(c) * delta, delta


# ---- the kernel's rounding points, in numpy fp32 ---------------------------------------------------------------------------
def _fmaf(a, b, c):
    """round32(a * b + c): the product of two fp32 values is exact in fp64; the sum is rounded to fp64 and then to fp32"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _axis32(d, t32, axis):
    n = d.shape[axis]
    r = len(t32) // 2
    idx = np.arange(n)
    acc = np.zeros_like(d, dtype=np.float32)
    norm = np.zeros_like(d, dtype=np.float32)
    shape = [1] * d.ndim
    shape[axis] = n
    for j in range(2 * r + 1):
        q = idx + j - r
        inside = ((q >= 0) & (q < n)).astype(np.float32).reshape(shape)
        t = np.float32(t32[j]) * inside                                    # (t * 1 and t * 0 are exact)
        v = np.take(d, np.clip(q, 0, n - 1), axis=axis)
        acc = _fmaf(np.broadcast_to(t, d.shape), v, acc)
        norm = (norm + t).astype(np.float32)
    return (acc / norm).astype(np.float32)


def lowpass32(d, sigma):
    d = np.asarray(d, dtype=np.float32)
    if radius(sigma) == 0:
        return d
    t32 = taps64(sigma).astype(np.float32)
    return _axis32(_axis32(d, t32, d.ndim - 1), t32, d.ndim - 2)


def correct32(x0, z, prev, w, c, sigma):
    """fp32 tensors -> (x0', prev') as fp32 tensors, every operation rounded where the kernel rounds"""
    x0n, zn, pn = (t.detach().cpu().numpy().astype(np.float32) for t in (x0, z, prev))
    w, c = np.float32(w), np.float32(c)
    delta = (w * lowpass32((zn - x0n).astype(np.float32), sigma)).astype(np.float32)
    return torch.from_numpy((x0n + delta).astype(np.float32)), torch.from_numpy((pn + (c * delta).astype(np.float32)).astype(np.float32))


def bound(z, x0, w, c, sigma):
    """K * 2^-24 * (max|z| + max|x0|) * |w| * (1 + |c|), K = 4 k + 8 for k = 2 r + 1 taps per axis (DESIGN.md section 7 "LQ
    fidelity" has the derivation; it presumes |w| >= 1/2 and max|prev| <= max|z| + max|x0|, which the tests assert of their inputs)."""
    k = 2 * radius(sigma) + 1
    D = float(z.abs().max()) + float(x0.abs().max())
    return (4 * k + 8) * 2.0 ** -24 * D * abs(float(w)) * (1.0 + abs(float(c)))


# ---- the cases of the kernel tests (CPU: the fp32 restatement inside the bound; GPU: the kernel) -----------------------------------
KERNEL_SHAPES = [(2, 4, 17, 23), (1, 4, 16, 16), (1, 4, 37, 67)]       # (the last: 32 + 5 rows, 2 * 32 + 3 columns of the built tile)
KERNEL_SIGMAS = [0.0, 0.5, 1.5, 8.0]
KERNEL_WC = [(0.75, 0.625), (1.0, -1.375)]                             # |w| >= 1/2, c of either sign


def kernel_case(shape, seed=0):
    """(x0, z, prev) fp32 of a kernel test: unit-variance planes, so max|prev| <= max|z| + max|x0| as `bound` presumes"""
    g = torch.Generator().manual_seed(100 + seed)
    x0, z, prev = (torch.randn(*shape, generator=g) for _ in range(3))
    assert prev.abs().max() <= z.abs().max() + x0.abs().max()
    return x0, z, prev


def bound32(z, x0, c):
    """What the kernel may differ by from `correct32`, which rounds where the kernel rounds: nothing but the restatement's fmaf
    (a sum rounded to fp64 and then to fp32 can land one fp32 ulp beside the fused result) and the order hipcc gives no say
    over; one ulp of a value of magnitude D = max|z| + max|x0|, 2^-23 D, on x0', and (1 + |c|) times that on prev'."""
    D = float(z.abs().max()) + float(x0.abs().max())
    return 2.0 ** -23 * D, 2.0 ** -23 * D * (1.0 + abs(float(c)))


# ---- the method as a guide hook ---------------------------------------------------------------------------------------------
def fidelity(base, z, w, decay, sigma):
    """guide(rows, i, t, x, coef) -> e - (sa / sb) delta, with e = base(rows, i, t, x, coef), x0 = (x - sb e) / sa,
    delta = w_i LP(z - x0), w_i = w (s_i / s_0) ** decay rounded to fp32 as the host does, s = sb / sa, s_0 taken from the
    `coef` of the hook's first call."""
    state = {}

    def guide(rows, i, t, x, coef):
        e = base(rows, i, t, x, coef)
        sb, sa = float(coef[0]), float(coef[1])
        s = sb / sa
        state.setdefault("s0", s)
        w_i = float(np.float32(float(w) if decay == 0 else float(w) * (s / state["s0"]) ** float(decay)))
        x0 = (x.double() - sb * e.double()) / sa
        delta = w_i * lowpass(z.double() - x0, sigma)
        return (e.double() - (sa / sb) * delta).to(e.dtype)
    return guide
