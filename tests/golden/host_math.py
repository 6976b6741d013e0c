"""Fingerprint of this host's float32 exp / sin / cos / sqrt, shared by the golden generator and the tests.

torch runs these through MKL, whose code path -- and so the last ulp of its results -- depends on the CPU vendor.  The
generator records the fingerprint of the host that produced the goldens (host_math.json); a test that compares the
oracle with a golden bit for bit (or at 1e-6) does so where this host's fingerprint is the same, and otherwise allows
only what a few-ulp difference in these functions carries through the computation it checks.
"""
from __future__ import annotations

import hashlib
import json
import os

import numpy as np
import torch

ULPS = 2.0 ** -21        # 4 float32 ulps (relative): the slack granted per transcendental on a host whose math differs


def _inputs():
    g = torch.Generator().manual_seed(20)
    u = torch.rand(100000, generator=g)
    return {"exp": -10 * u, "sin": 1000 * u, "cos": 1000 * u, "sqrt": u}


def fingerprint():
    return {f: hashlib.sha256(getattr(torch, f)(x).numpy().tobytes()).hexdigest() for f, x in _inputs().items()}


def same_as_golden_host(golden_dir):
    with open(os.path.join(golden_dir, "host_math.json")) as f:
        return fingerprint() == json.load(f)


def lcm_step_slack(alpha_cumprod, x, eps):
    """|error| a few-ulp sqrt(a) / sqrt(1 - a) difference carries through (x - sqrt(1 - a) eps) / sqrt(a), and so into
    c_out * x0 + c_skip * x (c_out <= 1) and sqrt(a) x + sqrt(1 - a) eps."""
    a = float(alpha_cumprod)
    return ULPS * (np.abs(x) + (1 - a) ** 0.5 * np.abs(eps)) / a ** 0.5


def sinusoid_slack(t, dim):
    """|error| a few-ulp exp (frequencies) and sin / cos difference carries into [cos(t f), sin(t f)]."""
    half = dim // 2
    ang = np.abs(np.asarray(t, np.float64)).reshape(-1, 1) * np.exp(-np.log(10000) * np.arange(half) / half)[None, :]
    return np.tile(ULPS * (ang + 1), 2)
