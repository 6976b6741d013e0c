"""CPU: the fp64 reference of csrc/norm.hip and its bound (tests/norm_ref.py) checked without a GPU.

  * at zero slack the reference is F.group_norm / F.layer_norm / torch.softmax in float64 (1e-12), at every case of the GPU file;
  * the numpy fp32 stand-ins of the kernels -- the kernels' arithmetic in their own order, once with and once without fused
    multiply-adds -- have 0 elements outside the bound at every one of them;
  * every mutant of a stand-in (one deliberate fault each) leaves the bound at the cases named here, and a mutant that cannot touch
    a case changes no bit there;
  * under the host formulas of `iir_groupnorm_nhwc` (`norm_ref.gn_geo`) the case table reaches every branch of the kernels (the list is in `test_case_table_reaches_every_branch`).
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import norm_ref as R

NAMES = list(R.CASES)


@functools.lru_cache(maxsize=None)
def checked(name):
    """(elements outside, worst ratio) of the fused and of the unfused stand-in; the reference is computed once for both."""
    cs = R.CASES[name]
    ref = R.reference(cs)
    assert (ref.lo <= ref.want).all() and (ref.want <= ref.hi).all()
    mask = R.written_mask(cs)
    return tuple(R.compare(R.standin(cs, fused), ref, mask) for fused in (True, False))


@pytest.mark.parametrize("name", NAMES)
def test_standin_is_inside_the_bound(name):
    (n1, r1), (n0, r0) = checked(name)
    print(f"{name}: stand-in worst err / bound {r1:.3f} fused, {r0:.3f} unfused")
    assert n1 == 0 and n0 == 0, (name, n1, n0)


def _torch_reference(cs):
    o = cs.opt
    if cs.kind in ("gn", "gnp"):
        Rr, HW, C, G = cs.shape
        _, v, gm, bt = R.gn_input(cs.shape, cs.dtype, o["mode"])
        x = torch.from_numpy(v).permute(0, 2, 1)
        y = F.group_norm(x, G, gm.double(), bt.double(), o["eps"]).permute(0, 2, 1)
        return (F.silu(y) if o["silu"] else y).reshape(Rr * HW, C).numpy()
    if cs.kind == "ln":
        rows, C = cs.shape
        _, x, gm, bt, sh, sc = R.ln_input(cs.shape)
        g = gm[0].double() if "g" in o["affine"] else None
        b = bt[0].double() if "b" in o["affine"] else None
        if g is None and b is not None:
            y = F.layer_norm(torch.from_numpy(x), (C,), None, None, o["eps"]) + b
        else:
            y = F.layer_norm(torch.from_numpy(x), (C,), g, b, o["eps"])
        if o.get("ada"):
            m = torch.arange(rows) // o["rpm"]
            y = y * (1 + sc[0].double()[m]) + sh[0].double()[m]
        y = y.numpy()
        return R._transpose(y, o, 0.0) if o.get("tr") else y
    x = torch.from_numpy(R.sm_input(cs.kind, cs.shape)[1])
    return torch.softmax(x, dim=-1).numpy()


@pytest.mark.parametrize("name", [n for n in NAMES if not (R.CASES[n].kind == "gnp")])
def test_reference_at_zero_slack_is_torch_in_float64(name):
    cs = R.CASES[name]
    got, want = R.reference(cs, rounding=False), _torch_reference(cs)
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, float(np.abs(want).max())), float(np.abs(got - want).max())


@pytest.mark.parametrize("name", [n for n in NAMES if R.CASES[n].kind == "gnp"])
def test_partials_reference_is_group_norm_up_to_the_fp32_partials(name):
    """The `partials=` reference takes the fp32-rounded partials as inputs, so it equals group_norm of x only up to their
    rounding: the mean moves by <= u A (u = 2^-24, A = max |mean_i|) and the variance by <= 2 u A Dp + u var (Dp the largest
    |mean_i - mean|), so an element by about (|x - mean| (u A Dp / var + u) + u A) |a|: below 1e-5 centred (A ~ 4, Dp ~ 3) and below
    1e-3 at a mean of 300 spreads."""
    cs = R.CASES[name]
    got, want = R.reference(cs, rounding=False), _torch_reference(cs)
    tol = 1e-5 if cs.opt["mode"] == "c" else 1e-3
    assert np.abs(got - want).max() <= tol * max(1.0, float(np.abs(want).max()))


# mutant -> (cases it must leave the bound at, cases it must not change a bit of)
MUT = {
    "var_ex2": (["gn.2x2600x320g32.f16.lin.e6.lm1000"], []),
    "var_nm1": (["gn.1x1x64g32.f16.lin.e5", "gn.1x7x64g64.bf16.silu.e6"], []),
    "eps_after_sqrt": (["gn.3x100x960g32.f16.lin.e5.tiny", "gn.3x100x960g32.bf16.silu.e6.tiny"], []),
    "last_slab_full": (["gn.3x100x960g32.f16.silu.e5", "gn.64x250x320g32.bf16.lin.e6", "gn.2x2600x320g32.f16.silu.e5.lm300", "gn.1x2041x64g32.f16.silu.e5"],
                       ["gn.64x256x64g4.f16.silu.e5", "gn.1x64x2560g32.f16.lin.e5"]),
    "tail_dropped": (["gn.3x100x960g32.f16.silu.e5", "gn.64x250x320g32.f16.silu.e6", "gn.1x4100x960g32.f16.silu.e5",
                      "gn.2x328x2560g32.bf16.lin.e5"],
                     ["gn.1x1x64g32.f16.lin.e5", "gn.1x7x64g64.f16.lin.e5"]),          # one pixel per thread: its first sample is the mean either way
    "nt_off_by_one": (["gn.3x100x960g32.f16.silu.e5", "gn.64x250x320g32.f16.lin.e5", "gn.1x4100x72g12.f16.silu.e6.lm300", "gn.1x4100x960g32.bf16.lin.e6"],
                      ["gn.1x64x2560g32.f16.lin.e5", "gn.2x328x2560g32.bf16.lin.e5"]),
    "slabs_beyond_32": (["gn.2x2600x320g32.f16.silu.e5", "gn.1x4100x72g12.bf16.lin.e6", "gn.2x328x2560g32.f16.silu.e5", "gn.1x2041x64g32.bf16.lin.e6"],
                        ["gn.3x100x960g32.f16.silu.e5", "gn.64x256x64g4.bf16.lin.e6"]),
    "group_from_chunk": (["gn.1x1x64g32.f16.silu.e5", "gn.1x7x64g64.f16.lin.e6", "gn.1x4100x72g12.f16.lin.e5", "gn.64x250x320g32.bf16.silu.e5",
                          "gn.3x100x960g32.f16.lin.e5.lm300", "gnp.1x64x64g64.f16.silu.e5", "gnp.2x32768x80g8.bf16.lin.e6"],
                         ["gn.64x256x64g4.f16.silu.e5", "gn.1x64x2560g32.bf16.lin.e6"]),
    "gi_mask_dropped": (["gn.64x256x64g4.f16.silu.e5", "gn.64x256x64g4.bf16.lin.e6"], ["gn.2x2600x320g32.f16.silu.e5", "gn.1x4100x72g12.f16.lin.e5"]),
    "silu_before_affine": (["gn.3x100x960g32.f16.silu.e5", "gn.1x1x64g32.bf16.silu.e6", "gnp.2x1024x320g32.f16.silu.e5"], ["gn.3x100x960g32.f16.lin.e5"]),
    "ldx_for_ldy": (["gn.1x7x64g64.f16.lin.e5", "gn.3x100x960g32.bf16.silu.e5", "gnp.2x1024x320g32.f16.silu.e5"], ["gn.1x1x64g32.f16.lin.e5"]),
    "stale_workspace": (["gn.2x2600x320g32.f16.silu.e5", "gn.1x4100x72g12.bf16.lin.e6", "gn.1x4100x960g32.f16.silu.e5"],
                        ["gn.3x100x960g32.f16.silu.e5", "gn.1x2041x64g32.f16.silu.e5"]),
    "cols_true_slab_len": (["gnp.1x64x64g64.f16.silu.e5", "gnp.2x16448x64g64.bf16.lin.e6", "gnp.2x32768x80g8.f16.silu.e5", "gnp.2x1024x320g32.f16.lin.e6.lm300"], []),
    "ln_mean_full_pass": (["ln.c8.r1.gb", "ln.c64.r5.none", "ln.c504.r37.g", "ln.c520.r37.b", "ln.c1280.r5.gb", "ln.c2552.r37.gb", "ln.fp8.c8"],
                          ["ln.c512.r37.gb", "ln.c2048.r5.g", "ln.c2560.r37.none"]),
    "ln_eps_after_sqrt": (["ln.c8.r37.gb"], []),
    "ln_scale_no_one": (["ln.ada.c8", "ln.ada.c520", "ln.tr.c2560"], ["ln.c520.r37.gb"]),
    "ln_shift_scale_swapped": (["ln.ada.c8", "ln.ada.c2552", "ln.tr.c504"], ["ln.c8.r5.g"]),
    "ln_mod_row_modulo": (["ln.ada.c64", "ln.ada.c2560", "ln.tr.c8"], ["ln.c64.r37.b"]),
    "ln_tr_no_bstride": (["ln.tr.c8", "ln.tr.c520", "ln.tr.c2560"], ["ln.ada.c520"]),
    "ln_fp8_from_fp32": (["ln.fp8.c2560", "ln.fp8.c2048"], ["ln.c2560.r37.gb"]),
    "sm_max_one_wave": (["sm16.c2040", "sm16.c16384", "sm32.c4100.f16", "sm32.c16380.bf16"], ["sm16.c8", "sm32.c4.f16"]),
    "sm_sum_one_wave": (["sm16.c2048", "sm16.c2056", "sm32.c4092.bf16", "sm32.c16384.f16"], ["sm16.c8", "sm32.c4.bf16"]),
    "sm_clamped_dup": (["sm16.c8", "sm16.c2040", "sm16.c2056", "sm16.c16376", "sm32.c4.f16", "sm32.c4096.bf16", "sm32.c16380.f16"],
                       ["sm16.c16384", "sm32.c16384.f16", "sm32.c16384.bf16"]),
    "sm_bf16_trunc": (["sm32.c4.bf16", "sm32.c4100.bf16", "sm32.c16384.bf16"], ["sm32.c4100.f16", "sm32.c16384.f16"]),
}


def test_every_mutant_is_listed():
    assert set(MUT) == set(R.MUTANTS)
    for mut, (out, inert) in MUT.items():
        assert out and all(n in R.CASES for n in out + inert), mut


@pytest.mark.parametrize("mut,name", [(m, n) for m, (out, _) in MUT.items() for n in out])
def test_mutant_leaves_the_bound(mut, name):
    cs = R.CASES[name]
    ref, mask = R.reference(cs), R.written_mask(cs)
    for fused in (True, False):
        n, ratio = R.compare(R.standin(cs, fused, mut), ref, mask)
        print(f"{mut} at {name} ({'fused' if fused else 'unfused'}): {n} elements outside, worst err / bound {ratio:.3g}")
        assert n > 0, (mut, name, fused)


@pytest.mark.parametrize("mut,name", [(m, n) for m, (_, inert) in MUT.items() for n in inert])
def test_mutant_that_cannot_touch_a_case_changes_no_bit(mut, name):
    cs = R.CASES[name]
    assert np.array_equal(R.standin(cs, True, mut), R.standin(cs, True), equal_nan=True)


def test_case_table_reaches_every_branch():
    geos = {n: R.gn_geo(*c.shape) for n, c in R.CASES.items() if c.kind == "gn"}
    some = lambda f: [n for n, g in geos.items() if f(g)]
    assert some(lambda g: g.pps < 8) and some(lambda g: g.pps == 8) and some(lambda g: g.pps > 8)
    assert some(lambda g: g.loop4 == {0}) and some(lambda g: 1 in g.loop4) and some(lambda g: max(g.loop4) >= 2)
    assert some(lambda g: max(g.loop4) >= 2 and g.prows > 1 and g.cnt > 8), "the 4-deep loop twice with a tail after it"
    assert some(lambda g: g.last < g.pps)
    assert some(lambda g: g.nslab == 1) and some(lambda g: 33 <= g.nslab <= 255 and g.nslab % 32) and some(lambda g: g.nslab == 256)
    assert some(lambda g: g.nslab > 32 and g.last < g.pps), "slots k >= 1 of a finalize lane with a short last slab"
    assert some(lambda g: g.nslab0 > g.nslab), "a first slab estimate above the final one"
    assert some(lambda g: g.prows == 1) and some(lambda g: g.prows > 1 and g.idle)
    assert some(lambda g: g.passes == 2)
    assert {1, 10, 80} <= {g.cpg for g in geos.values()}
    assert {4, 12, 32, 64} <= {c.shape[3] for c in R.CASES.values() if c.kind == "gn"}
    assert {1, 2, 4} <= {g.gblocks for g in geos.values()}
    assert {c.dtype for c in R.CASES.values() if c.kind == "gn"} == {"f16", "bf16"}
    for shape in R.GN_SHAPES:                       # every base shape at both types, SiLU on and off, both eps
        have = {(c.dtype, c.opt["silu"], c.opt["eps"]) for c in R.CASES.values() if c.kind == "gn" and c.shape == shape and c.opt["mode"] == "c"}
        assert len(have) == 8, shape
    assert {"lm300", "lm1000", "tiny"} <= {c.opt["mode"] for c in R.CASES.values() if c.kind == "gn"}
    ns = {(c.shape[1] // 64) * (c.shape[2] // c.shape[3]) for c in R.CASES.values() if c.kind == "gnp"}
    assert {1, 257, 5120} <= ns and {c.dtype for c in R.CASES.values() if c.kind == "gnp"} == {"f16", "bf16"}
    ln = [c for c in R.CASES.values() if c.kind == "ln"]
    assert {c.shape[1] for c in ln} == set(R.LN_CS) and {c.shape[0] for c in ln} >= {1, 5, 37}
    for C in R.LN_CS:
        assert {c.opt["affine"] for c in ln if c.shape[1] == C} == {"gb", "g", "b", ""}
        assert any(c.opt.get("ada") and c.shape[0] % 4 and c.shape[0] % c.opt["rpm"] for c in ln if c.shape[1] == C)
        assert any(c.opt.get("tr") and c.opt["tr_bstride"] > c.opt["tr_rows"] for c in ln if c.shape[1] == C)
        assert any(c.opt.get("fp8") for c in ln if c.shape[1] == C)
    assert {c.shape[1] for c in R.CASES.values() if c.kind == "sm16"} == set(R.SM16_COLS)
    assert {(c.shape[1], c.dtype) for c in R.CASES.values() if c.kind == "sm32"} == {(c, d) for c in R.SM32_COLS for d in ("f16", "bf16")}


def test_bound_names_what_grows_with_the_mean():
    """|mean| / spread is reported per case and the bound grows with it: the large-mean launch of a shape has the wider mean and
    rstd terms (the centred one is held up by its 6 D share, so the factor is below the ratio of the means)."""
    c = R.reference(R.CASES["gn.3x100x960g32.f16.lin.e5"]).terms
    m = R.reference(R.CASES["gn.3x100x960g32.f16.lin.e5.lm300"]).terms
    assert m["mean_over_sigma"] > 250 and c["mean_over_sigma"] < 5
    assert m["rstd_rel"] > 5 * c["rstd_rel"] and m["e_mean_over_sigma"] > 5 * c["e_mean_over_sigma"]


def test_roundings():
    x = np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), 3.0e-5, 0.0, 65520.0])
    assert np.array_equal(R.rnd(x, "bf16")[:3], [1.0, 1.0 + 2.0 ** -6, -1.0])          # ties to even
    assert np.array_equal(R.rnd(x, "bf16"), torch.from_numpy(x).float().bfloat16().double().numpy())
    assert R.rnd(x, "f16")[3] == float(np.float16(3.0e-5)) and np.isinf(R.rnd(x, "f16")[5])
