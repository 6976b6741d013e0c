"""CPU: LQ fidelity guidance without a GPU -- the fp64 restatement against a brute-force loop, the host tables (w_i, c_i), the
argument checks, the C entry's binding and refusals, the `guide` hook of the restatement against the step arithmetic, and the
derived bound against an fp32 restatement with the kernel's rounding points."""
import ctypes
import math
import re

import numpy as np
import pytest
import torch

import loop_ref as lr
import lq_fidelity_ref as ref
from instantir_amd import lib
from instantir_amd import lq_fidelity as lqf


# ---- the restatement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [0.5, 1.5, 8.0])
def test_lowpass_matches_a_double_loop(sigma):
    H, W = 5, 7
    d = torch.randn(H, W, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    r = math.ceil(3 * sigma)
    g = [math.exp(-((j - r) ** 2) / (2 * sigma * sigma)) for j in range(2 * r + 1)]
    want = torch.zeros(H, W, dtype=torch.float64)
    for y in range(H):
        for x in range(W):
            num = den = 0.0
            for jy in range(-r, r + 1):
                for jx in range(-r, r + 1):
                    if 0 <= y + jy < H and 0 <= x + jx < W:
                        wgt = g[jy + r] * g[jx + r]
                        num += wgt * d[y + jy, x + jx].item()
                        den += wgt
            want[y, x] = num / den
    assert (ref.lowpass(d, sigma) - want).abs().max().item() < 1e-13


@pytest.mark.parametrize("sigma", [0.0, 0.25, 1.5, 8.0])
def test_lowpass_keeps_a_constant_at_the_corners(sigma):
    out = ref.lowpass(torch.full((2, 9, 6), 3.25, dtype=torch.float64), sigma)
    for y, x in ((0, 0), (0, 5), (8, 0), (8, 5), (4, 3)):
        assert abs(out[1, y, x].item() - 3.25) < 1e-14
    out32 = ref.lowpass32(np.full((2, 9, 6), 3.25, dtype=np.float32), sigma)
    assert np.abs(out32 - 3.25).max() <= 4 * 3.25 * 2.0 ** -23


def test_product_taps_are_the_restatements():
    for sigma in (0.25, 0.5, 1.5, 8.0):
        t = lqf.taps(sigma)
        assert len(t) == 2 * lqf.radius(sigma) + 1 == 2 * ref.radius(sigma) + 1
        assert np.abs(np.array(t) - ref.taps64(sigma)).max() < 1e-15 and abs(math.fsum(t) - 1.0) < 1e-15
    assert lqf.taps(0.0) == [] and lqf.radius(0.0) == 0
    assert lqf.radius(8.0) == lqf.MAX_RADIUS == 24 and lqf.radius(0.25) == 1


# ---- w_i ---------------------------------------------------------------------------------------------------------------------
def _ddim30():
    from instantir_amd.schedulers import DDIMScheduler
    s = DDIMScheduler()
    s.set_timesteps(30)
    ts = [int(t) for t in s.timesteps]
    return s, ts


def _euler_karras(n=12):
    s = lr.sigma_sched("euler", karras=True)
    s.set_timesteps(n)
    return s, [float(t) for t in s.timesteps]


@pytest.mark.parametrize("table", [_ddim30, _euler_karras])
def test_weight_table(table):
    s, ts = table()
    coefs = lqf.step_coefs(s, ts)
    assert len(coefs) == len(ts)
    for decay in (0.5, 2.0, 4.0):
        rows = lqf.tables(coefs, 0.8, decay)
        w = [r[0] for r in rows]
        assert w[0] == float(np.float32(0.8))
        assert all(a >= b for a, b in zip(w, w[1:])) and w[-1] < w[0]
        assert decay < 2 or w[-1] < 0.01 * w[0]                          # the ratio's own square: gone at the end
        s0 = coefs[0][1] / coefs[0][2]
        for cf, wi in zip(coefs, w):
            assert wi == float(np.float32(0.8 * ((cf[1] / cf[2]) / s0) ** decay))
    flat = lqf.tables(coefs, 0.3, 0.0)
    assert {r[0] for r in flat} == {float(np.float32(0.3))}
    # a call cut short (denoising_end) or resumed takes s_0 from ITS first step
    tail = lqf.tables(coefs[5:], 0.8, 2.0)
    assert tail[0][0] == float(np.float32(0.8)) and len(tail) == len(ts) - 5


# ---- c_i: the corrected prev is the step run on e' ---------------------------------------------------------------------------
def _family(name):
    from instantir_amd import schedulers as S
    if name == "ddim":
        s = S.DDIMScheduler()
    elif name == "ddim_eta":
        s = S.DDIMScheduler()
    elif name == "ddpm":
        s = S.DDPMScheduler()
    else:
        s = lr.sigma_sched(name)
    s.set_timesteps(8)
    hist = hasattr(s, "loop_coefficients")
    ts = [float(t) if hist else int(t) for t in s.timesteps]
    return lqf.step_coefs(s, ts, eta=0.7 if name == "ddim_eta" else 0.0)


@pytest.mark.parametrize("name", ["ddim", "ddim_eta", "ddpm", "euler", "euler_a", "dpm", "dpm_sde"])
def test_prev_gain_is_the_step_on_the_corrected_eps(name):
    g = torch.Generator().manual_seed(5)
    coefs = _family(name)
    e, x, m, nz, z = (torch.randn(2, 4, 6, 5, generator=g, dtype=torch.float64) for _ in range(5))
    seen_second_order = False
    for i, cf in enumerate(coefs):
        seen_second_order |= cf[7] != 0.0
        c = lqf.prev_gain(cf)
        assert c == float(np.float32(c))
        sb, sa = cf[1], cf[2]
        prev, x0 = lr.ref_step(e, x, cf, m, nz)
        assert prev.dtype == torch.float64
        x0n, prevn, delta = ref.correct(x0, z, prev, 0.6, c, 1.5)
        prev_e, x0_e = lr.ref_step(e - (sa / sb) * delta, x, cf, m, nz)
        scale = max(prev_e.abs().max().item(), 1.0)
        assert (x0_e - x0n).abs().max().item() < 1e-12 * scale, (name, i)
        assert (prev_e - prevn).abs().max().item() < 2.0 ** -23 * scale, (name, i)     # c is rounded to fp32, nothing else is
    assert seen_second_order == (name in ("dpm", "dpm_sde"))
    assert lqf.prev_gain([0, 0.0, 1.0, 1.0, 0, 0.0, 0, 0]) == 1.0                         # k_eps == 0: k_x0, whatever sb is


def test_guide_hook_returns_the_eps_whose_step_is_the_corrected_one():
    """`ref.fidelity` around `cfg_guide`: the eps it returns gives x0 + delta through `ref_step`, with w_i from the first call's
    ratio (the form the oracle loops take the method in)."""
    g = torch.Generator().manual_seed(9)
    u, c, x, z = (torch.randn(2, 4, 6, 5, generator=g, dtype=torch.float64) for _ in range(4))
    coefs = _family("ddim")
    hook = ref.fidelity(lr.cfg_guide(7.0), z, 0.6, 2.0, 1.5)
    rows = lqf.tables(coefs, 0.6, 2.0)
    for i in (0, 3, 7):                                    # (the first call fixes s_0: step 0 comes first)
        cf = coefs[i]
        e = u + 7.0 * (c - u)
        e_fid = hook((u, c), i, None, x, (cf[1], cf[2]))
        _, x0 = lr.ref_step(e, x, cf, None, None)
        _, x0_fid = lr.ref_step(e_fid, x, cf, None, None)
        want, _, _ = ref.correct(x0, z, x0, rows[i][0], 0.0, 1.5)
        assert (x0_fid - want).abs().max().item() < 1e-12 * max(want.abs().max().item(), 1.0), i


# ---- validation ----------------------------------------------------------------------------------------------------------------
def test_check_accepts_and_switches_off():
    assert lqf.check(None) is None and lqf.check(0) is None and lqf.check(0.0, 3.0, 1.5) is None
    assert lqf.check(0.5) == (0.5, 2.0, 0.0) and lqf.DEFAULT_DECAY == 2.0
    assert lqf.check(1, 0, 0.25) == (1.0, 0.0, 0.25)
    assert lqf.check(np.float32(0.5), 1.5, 8) == (0.5, 1.5, 8.0)


@pytest.mark.parametrize("args", [(-0.1,), (1.01,), (float("nan"),), (float("inf"),), ("0.5",), (True,),
                                  (0.5, -1.0), (0.5, float("inf")), (0.5, float("nan")), (0.5, None), (0.5, "2"),
                                  (0.5, 2.0, -1.0), (0.5, 2.0, 0.2), (0.5, 2.0, 8.5), (0.5, 2.0, float("nan")), (0.5, 2.0, None),
                                  (None, -1.0), (None, 2.0, 0.1), (0, 2.0, 9.0)])
def test_check_refuses(args):
    with pytest.raises(ValueError, match="lq_fidelity"):
        lqf.check(*args)


# ---- binding, entry ------------------------------------------------------------------------------------------------
def test_entry_is_declared_bound_and_exported():
    assert "iir_lq_fidelity_f32" in lib.declared_symbols()
    P, I = ctypes.c_void_p, ctypes.c_int32
    assert lib.SIGNATURES["iir_lq_fidelity_f32"] == (ctypes.c_int, [P, P, P, I, P, I, I, I, P, P, P, P])
    assert hasattr(ctypes.CDLL(lib.LIB_PATH), "iir_lq_fidelity_f32")
    assert lib.load().iir_abi_version() == 3
    from instantir_amd import ops
    header = open(lib.HEADER_PATH).read()
    assert int(re.search(r"#define IIR_LQ_FIDELITY_MAX_RADIUS (\d+)", header).group(1)) == ops.LQ_FIDELITY_MAX_RADIUS == lqf.MAX_RADIUS
    assert int(re.search(r"#define IIR_LQ_FIDELITY_TILE (\d+)", header).group(1)) == ops.LQ_FIDELITY_TILE
    assert lqf.radius(lqf.MAX_LOWPASS) == lqf.MAX_RADIUS


X0, LQ, TAPS, WC, PREV, OUT, HIST = (0x10000 * (i + 1) for i in range(7))      # never dereferenced: every case is refused first
GOOD = dict(x0=X0, lq=LQ, taps=TAPS, r=4, wc=WC, planes=8, H=17, W=23, prev=PREV, out=OUT, hist=HIST)
BAD = {
    "null x0": dict(x0=None), "null lq": dict(lq=None), "null wc": dict(wc=None), "null prev": dict(prev=None), "null out": dict(out=None),
    "radius 25": dict(r=25), "radius -1": dict(r=-1), "null taps": dict(taps=None), "planes 0": dict(planes=0), "planes -3": dict(planes=-3),
    "planes 65536": dict(planes=65536), "H 0": dict(H=0), "W 0": dict(W=0), "H -1": dict(H=-1), "W 32769": dict(W=32769),
    "out is x0": dict(out=X0), "out is x0, radius 0": dict(out=X0, r=0, taps=None), "out is lq": dict(out=LQ), "prev is x0": dict(prev=X0),
    "prev is lq": dict(prev=LQ), "prev is out": dict(prev=OUT), "hist is x0": dict(hist=X0), "hist is lq": dict(hist=LQ),
    "hist is prev": dict(hist=PREV), "hist is out": dict(hist=OUT),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_entry_refuses_before_any_hip_call(case):
    a = dict(GOOD, **BAD[case])
    rc = lib.load().iir_lq_fidelity_f32(a["x0"], a["lq"], a["taps"], a["r"], a["wc"], a["planes"], a["H"], a["W"], a["prev"], a["out"],
                                        a["hist"], None)
    assert rc == -1, (case, rc)


# ---- the derived bound holds for an fp32 restatement with the kernel's rounding points -------------------------------------------
@pytest.mark.parametrize("sigma", ref.KERNEL_SIGMAS)
@pytest.mark.parametrize("shape", ref.KERNEL_SHAPES)
def test_fp32_restatement_stays_inside_the_derived_bound(shape, sigma):
    from instantir_amd import ops
    T = ops.LQ_FIDELITY_TILE
    assert ref.KERNEL_SHAPES[2][2] == T + 5 and ref.KERNEL_SHAPES[2][3] == 2 * T + 3
    x0, z, prev = ref.kernel_case(shape)
    for w, c in ref.KERNEL_WC:
        want_x0, want_prev, _ = ref.correct(x0, z, prev, np.float32(w), np.float32(c), sigma)
        got_x0, got_prev = ref.correct32(x0, z, prev, w, c, sigma)
        tol = ref.bound(z, x0, w, c, sigma)
        e0, e1 = (got_x0.double() - want_x0).abs().max().item(), (got_prev.double() - want_prev).abs().max().item()
        print(f"{shape} sigma {sigma} w {w} c {c}: fp32 restatement |err| x0' {e0:.3e} prev' {e1:.3e}, bound {tol:.3e}")
        assert e0 <= tol and e1 <= tol
