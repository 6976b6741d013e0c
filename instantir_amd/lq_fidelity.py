"""Host side of LQ fidelity guidance (DESIGN.md section 7 "LQ fidelity"): what `ops.lq_fidelity` needs from the host.  The denoising
loop does not call it yet (DESIGN.md says why); a caller that runs its own loop over `scheduler.step` can.

After every main-UNet evaluation the step's predicted clean latent x0 is pulled toward the LQ latent z -- strongly at high
noise, not at all at the end -- the restoration-guided sampling of SUPIR (over the whole band) and the low-frequency
refinement of ILVR (through a low-pass) stated on this loop's step:

    w_i  = lq_fidelity * (s_i / s_0) ** lq_fidelity_decay         s_i = sb_i / sa_i, the step's noise-to-signal ratio
    d    = w_i * LP(z - x0);   x0' = x0 + d;   prev' = prev + c_i * d,   c_i = k_x0 - k_eps * sa_i / sb_i

c_i is what running the step on e' = e - (sa / sb) d would have added to prev, so the correction is exact for every scheduler
whose update is prev = k_x0 x0 + k_x x + k_eps e + k_h m + k_noise n.  Everything here is plain host arithmetic in fp64: the
argument checks, the two per-step scalars the kernel reads, and the taps of LP."""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .lib import MACROS

DEFAULT_DECAY = 2.0
MAX_RADIUS = MACROS["IIR_LQ_FIDELITY_MAX_RADIUS"]     # ceil(3 sigma) of the largest low-pass the launch takes
MIN_LOWPASS, MAX_LOWPASS = 0.25, 8.0


def check(lq_fidelity, lq_fidelity_decay=DEFAULT_DECAY, lq_fidelity_lowpass=0.0) -> Optional[Tuple[float, float, float]]:
    """The three arguments of a call -> (weight, decay, lowpass sigma) as floats, or None when the feature is off (`lq_fidelity`
    None or 0; the other two are still checked).  ValueError for a weight outside [0, 1], a decay that is not finite and >= 0,
    a low-pass sigma that is neither 0 nor in [0.25, 8]."""
    def number(v, name):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError(f"{name} must be a number, got {v!r}")
        return float(v)

    decay = number(lq_fidelity_decay, "lq_fidelity_decay")
    if not math.isfinite(decay) or decay < 0.0:
        raise ValueError(f"lq_fidelity_decay must be finite and >= 0, got {lq_fidelity_decay!r}")
    sigma = number(lq_fidelity_lowpass, "lq_fidelity_lowpass")
    if not (sigma == 0.0 or MIN_LOWPASS <= sigma <= MAX_LOWPASS):
        raise ValueError(f"lq_fidelity_lowpass must be 0 (the whole band) or a Gaussian sigma in [{MIN_LOWPASS}, {MAX_LOWPASS}] latent "
                         f"pixels, got {lq_fidelity_lowpass!r}")
    if lq_fidelity is None:
        return None
    weight = number(lq_fidelity, "lq_fidelity")
    if not 0.0 <= weight <= 1.0:                     # (NaN fails both compares)
        raise ValueError(f"lq_fidelity must be None or a weight in [0, 1], got {lq_fidelity!r}")
    return (weight, decay, sigma) if weight > 0.0 else None


def radius(sigma: float) -> int:
    """r = ceil(3 sigma) taps on each side of the centre; 0 for sigma = 0 (LP is the identity)."""
    return int(math.ceil(3.0 * float(sigma)))


def taps(sigma: float) -> List[float]:
    """The 2 r + 1 Gaussian taps exp(-(j - r)^2 / (2 sigma^2)), normalised to sum 1, in fp64; [] for sigma = 0."""
    r = radius(sigma)
    if r == 0:
        return []
    if r > MAX_RADIUS:
        raise ValueError(f"lq_fidelity_lowpass {sigma} needs a radius of {r} taps, the launch takes {MAX_RADIUS}")
    g = [math.exp(-0.5 * ((j - r) / float(sigma)) ** 2) for j in range(2 * r + 1)]
    tot = math.fsum(g)
    return [v / tot for v in g]


def ratio(coef: Sequence[float]) -> float:
    """s = sb / sa of a step's coefficient vector {g, sb, sa, k_x0, k_x, k_eps, k_noise, k_h}."""
    return float(coef[1]) / float(coef[2])


def prev_gain(coef: Sequence[float]) -> float:
    """c = k_x0 - k_eps * sa / sb (k_x0 when k_eps == 0, which also covers sb == 0), fp64 rounded once to fp32."""
    sb, sa, k0, ke = (float(coef[j]) for j in (1, 2, 3, 5))
    return float(np.float32(k0 if ke == 0.0 else k0 - ke * sa / sb))


def tables(coefs: Sequence[Sequence[float]], weight: float, decay: float) -> List[Tuple[float, float]]:
    """(w_i, c_i) for the steps a call executes, `coefs` their coefficient vectors in order; s_0 is the first one's ratio.
    Each value is formed in fp64 and rounded once to fp32."""
    if not coefs:
        return []
    s0 = ratio(coefs[0])
    out = []
    for cf in coefs:
        # (s_0 == 0 cannot happen on a step that denoises; decay 0 gives the constant table whatever the ratios are)
        w = float(weight) if decay == 0.0 else float(weight) * (ratio(cf) / s0) ** float(decay)
        out.append((float(np.float32(w)), prev_gain(cf)))
    return out


def step_coefs(scheduler, ts, eta=0.0) -> List[List[float]]:
    """The coefficient vector of every loop step, as `_DenoiseLoop.step` forms it: `loop_coefficients(i)` of a sigma scheduler,
    `step_coefficients(t, eta=eta)` of DDPM / DDIM."""
    if hasattr(scheduler, "loop_coefficients"):
        return [list(scheduler.loop_coefficients(i)["coef"]) for i in range(len(ts))]
    return [list(scheduler.step_coefficients(t, eta=eta)) for t in ts]
