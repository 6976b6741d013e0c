"""Adaptive projected guidance (APG; Sadat et al., "Eliminating Oversaturation and Artifacts of High Guidance Scales in
Diffusion Models") restated in torch on CPU -- the executable form of the contract in include/instantir_hip.h, imported by
tests/test_apg_ref_cpu.py and tests/test_apg_gpu.py.  Nothing in the reference implements APG, so this file is the specification.

Per image b, sums over (C, H, W); u / c the uncond / cond predictions, x the unscaled latent, (w, sb, sa) = coef[0:3]:

    x0_c = (x - sb*c)/sa            x0_u = (x - sb*u)/sa
    D    = x0_c - x0_u
    A    = D + beta_t * A_prev      (skipped, A_prev not read, when beta_t == 0)
    n    = ||A||_2                  s = r > 0 ? min(1, r / n) : 1
    alpha= <A, x0_c> / <x0_c, x0_c>
    U    = s * (A - (1 - eta) * alpha * x0_c)
    x0_g = x0_c + (w - 1) * U
    eps  = (x - sa*x0_g)/sb

`apg_eps(..., fp32=False)` evaluates it in fp64.  `fp32=True` is the rounding-point restatement: the same statements with fp32
element math, fp64 accumulation of the three sums and {s, alpha} rounded to fp32 -- what a kernel with fp32 lanes computes, up
to fma contraction and summation order."""
import torch


def unpack_eps(eps16, rows, C, H, W):
    """(rows*H*W, lde) 16-bit NHWC rows -> fp64 (rows, C, H, W) of the values a kernel reads (columns [0, C))."""
    return eps16.double()[:, :C].reshape(rows, H, W, C).permute(0, 3, 1, 2).contiguous()


def apg_eps(u, c, x, a_prev, coef, eta, r, beta, fp32=False):
    """u, c, x, a_prev: (B, C, H, W); coef: the step's coefficient vector (w = coef[0], sb = coef[1], sa = coef[2]).
    -> (eps, A, s (B,), alpha (B,)) in fp64 (values of fp32 numbers when `fp32`)."""
    dt = torch.float32 if fp32 else torch.float64
    T = lambda v: torch.tensor(float(v), dtype=torch.float32).to(dt)      # scalars arrive as fp32 in either mode
    w, sb, sa = T(coef[0]), T(coef[1]), T(coef[2])
    eta, r32, beta = T(eta), T(r), T(beta)
    u, c, x = u.to(dt), c.to(dt), x.to(dt)
    B = x.shape[0]
    x0c = (x - sb * c) / sa
    x0u = (x - sb * u) / sa
    A = x0c - x0u
    if float(beta) != 0.0:
        A = A + beta * a_prev.to(dt)
    dims = (1, 2, 3)
    aa = (A.double() * A.double()).sum(dims)
    ac = (A.double() * x0c.double()).sum(dims)
    cc = (x0c.double() * x0c.double()).sum(dims)
    s = torch.ones(B, dtype=torch.float64)
    if float(r32) > 0.0:
        s = torch.minimum(s, r32.double() / aa.sqrt())
    alpha = ac / cc
    s, alpha = s.to(dt), alpha.to(dt)
    k = ((1 - eta) * alpha).view(B, 1, 1, 1)
    U = s.view(B, 1, 1, 1) * (A - k * x0c)
    x0g = x0c + (w - 1) * U
    eps = (x - sa * x0g) / sb
    return eps.double(), A.double(), s.double(), alpha.double()


def cfg_eps(u, c, w):
    """plain classifier-free guidance in fp64"""
    return u.double() + float(w) * (c.double() - u.double())


def step(eps, x, coef, m_prev=None, noise=None, fp32=False):
    """The scheduler update of iir_sched_step on a guided eps -> (prev, x0); terms with a zero coefficient are skipped."""
    dt = torch.float32 if fp32 else torch.float64
    _, sb, sa, k0, kx, ke, kn, kh = [torch.tensor(float(v), dtype=torch.float32).to(dt) for v in coef]
    eps, x = eps.to(dt), x.to(dt)
    x0 = (x - sb * eps) / sa
    pv = k0 * x0 + kx * x
    if float(ke) != 0:
        pv = pv + ke * eps
    if m_prev is not None and float(kh) != 0:
        pv = pv + kh * m_prev.to(dt)
    if noise is not None and float(kn) != 0:
        pv = pv + kn * noise.to(dt)
    return pv.double(), x0.double()
