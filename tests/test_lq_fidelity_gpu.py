"""GPU: the LQ fidelity launch (`ops.lq_fidelity`) element-wise against the fp64 restatement (tests/lq_fidelity_ref.py) inside the
derived bound and against the fp32 restatement with the kernel's rounding points inside one ulp of the operands' range, NaN guard
bands around every operand, two launches bit-equal, and the wrapper's refusals."""
import numpy as np
import pytest
import torch

import lq_fidelity_ref as ref
from loop_ref import dev  # noqa: F401  (fixture)
from lq_fidelity_ref import KERNEL_SHAPES, KERNEL_SIGMAS, KERNEL_WC, kernel_case

pytestmark = pytest.mark.gpu

GUARD = 4099                       # fp32 elements of NaN on either side of every operand (odd: the planes start 4-byte aligned only)


def _embedded(t, dev, fill=None):
    """A contiguous device tensor of t's shape in the middle of a larger allocation whose guard bands hold NaN bit patterns
    -> (view, whole buffer)"""
    n = t.numel()
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device=dev)
    view = buf[GUARD:GUARD + n].view(t.shape)
    view.copy_(t if fill is None else torch.full_like(t, fill))
    return view, buf


def _guards_intact(buf):
    return bool(torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[-GUARD:]).all())


def _taps(sigma, dev):
    from instantir_amd import lq_fidelity as lqf
    t = lqf.taps(sigma)
    return torch.tensor(t, dtype=torch.float64).to(torch.float32).to(dev) if t else None


def _launch(dev, x0, z, prev, w, c, sigma, with_hist):
    from instantir_amd import ops
    x0_d, b0 = _embedded(x0, dev)
    z_d, b1 = _embedded(z, dev)
    prev_d, b2 = _embedded(prev, dev)
    out_d, b3 = _embedded(x0, dev, fill=7.0)
    hist_d, b4 = _embedded(x0, dev, fill=-3.0) if with_hist else (None, None)
    wc, b5 = _embedded(torch.tensor([w, c], dtype=torch.float32), dev)
    ops.lq_fidelity(x0_d, z_d, wc, prev_d, out_d, taps=_taps(sigma, dev), hist=hist_d)
    torch.cuda.synchronize()
    assert all(_guards_intact(b) for b in (b0, b1, b2, b3, b5) + ((b4,) if with_hist else ()))
    assert torch.equal(x0_d.cpu(), x0) and torch.equal(z_d.cpu(), z)                   # the inputs keep their bits
    return out_d.cpu(), prev_d.cpu(), None if hist_d is None else hist_d.cpu()


@pytest.mark.parametrize("sigma", KERNEL_SIGMAS)
@pytest.mark.parametrize("shape", KERNEL_SHAPES)
def test_kernel_matches_fp64_inside_the_derived_bound(dev, shape, sigma):
    """x0', prev' and hist against the fp64 restatement on the same fp32 inputs (fp32 taps and scalars included in the budget),
    for c of either sign, with and without the history plane; two launches give equal bits.  Largest |error| / bound seen on an
    MI355X: 0.058, at sigma 0 (DESIGN.md section 7 "LQ fidelity").  That worst-case bound grows with the tap count and is
    loose at large radii, so the kernel is also held to `ref.correct32`, which rounds where the kernel rounds, within
    `ref.bound32` (one fp32 ulp of the operands' range, whatever the radius)."""
    x0, z, prev = kernel_case(shape)
    worst = 0.0
    for w, c in KERNEL_WC:
        want_x0, want_prev, _ = ref.correct(x0, z, prev, np.float32(w), np.float32(c), sigma)
        tol = ref.bound(z, x0, w, c, sigma)
        like_x0, like_prev = ref.correct32(x0, z, prev, w, c, sigma)
        tol32 = ref.bound32(z, x0, c)
        for with_hist in (False, True):
            got_x0, got_prev, got_hist = _launch(dev, x0, z, prev, w, c, sigma, with_hist)
            again = _launch(dev, x0, z, prev, w, c, sigma, with_hist)
            assert torch.isfinite(got_x0).all() and torch.isfinite(got_prev).all()
            assert torch.equal(got_x0, again[0]) and torch.equal(got_prev, again[1])
            e0, e1 = (got_x0.double() - want_x0).abs().max().item(), (got_prev.double() - want_prev).abs().max().item()
            print(f"{shape} sigma {sigma} w {w} c {c} hist {with_hist}: |err| x0' {e0:.3e} prev' {e1:.3e}, bound {tol:.3e}")
            worst = max(worst, e0 / tol, e1 / tol)
            assert e0 <= tol and e1 <= tol, (e0, e1, tol)
            d0, d1 = (got_x0 - like_x0).abs().max().item(), (got_prev - like_prev).abs().max().item()
            n0, n1 = int((got_x0 != like_x0).sum()), int((got_prev != like_prev).sum())
            print(f"    against the fp32 restatement: x0' {n0} of {got_x0.numel()} elements differ, max {d0:.3e} (allowed {tol32[0]:.3e}); "
                  f"prev' {n1}, max {d1:.3e} (allowed {tol32[1]:.3e})")
            assert d0 <= tol32[0] and d1 <= tol32[1], (d0, d1, tol32)
            if with_hist:
                assert torch.equal(got_hist, got_x0) and torch.equal(got_hist, again[2])
    print(f"{shape} sigma {sigma}: largest |error| / bound {worst:.3f}")


def test_ops_refuse_bad_arguments(dev):
    from instantir_amd import ops
    from instantir_amd.lib import HipLibraryError
    x0, z, prev = (t.to(dev) for t in kernel_case((1, 4, 8, 8)))
    out, wc = torch.empty_like(x0), torch.tensor([0.5, 0.5], device=dev)
    with pytest.raises(HipLibraryError):
        ops.lq_fidelity(x0, z, wc, prev, x0)                                           # x0_out == x0_in: refused by the entry
    with pytest.raises(ValueError, match="taps"):
        ops.lq_fidelity(x0, z, wc, prev, out, taps=torch.ones(4, device=dev))          # an even tap count
    with pytest.raises(ValueError, match="taps"):
        ops.lq_fidelity(x0, z, wc, prev, out, taps=torch.ones(51, device=dev))         # radius 25
    with pytest.raises(ValueError, match="lq"):
        ops.lq_fidelity(x0, z[:, :2], wc, prev, out)
    with pytest.raises(ValueError, match="wc"):
        ops.lq_fidelity(x0, z, wc.cpu(), prev, out)
