"""CPU: the references and bounds of tests/gemm_fused_ref.py (`ln_in`, `ln_out`, `gn_out`), checked without a GPU.

The `ln_in` reference with exact partials is fp64 LayerNorm -> Linear (-> GEGLU) up to the rounding of the partials to fp32; an
fp32 stand-in of each path, with the kernel's merge formulas and rounding points, leaves 0 elements outside the bound at every case
the GPU file runs; each mutant leaves it at every case where it is not the correct kernel (those cases are named); the acceptance
tables follow from the LDS formulas restated beside them."""
import functools

import pytest
import torch
import torch.nn.functional as F

import gemm_conv_ref as R
import gemm_fused_ref as FR

FORMS = ("f16", "bf16", "w8")


@functools.lru_cache(maxsize=None)
def ln_in_all():
    out = {}
    for form in FORMS:
        for n, c in FR.ln_in_cases(form).items():
            out[f"{form}.{n}"] = c
    for n, c in FR.ln_in_g8_cases().items():
        out[f"f16.{n}"] = c
    return out


@functools.lru_cache(maxsize=None)
def ln_in_ref(name):
    return R.reference(*ln_in_all()[name])


LN_IN_NAMES = sorted(ln_in_all())


def _parts(name):
    return ln_in_all()[name].spec["ln_in"][0].shape[0]


# ---- ln_in ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geglu", [False, True])
@pytest.mark.parametrize("parts", FR.LN_PARTS)
def test_ln_in_reference_is_layer_norm_then_linear_up_to_the_fp32_partials(parts, geglu):
    """With partials computed exactly from h, rstd (h w^T - mean colsum) + bias of the folded weight IS layer_norm(h) @ W^T + b in
    fp64 (and GEGLU of it): the two differ only by the rounding of the partials to fp32, which moves mean by 2^-24 |mean| and var by
    2^-23 var + 2 |d| 2^-24 |mean| -- carried to the output through rstd and |colsum|, the tolerance below, element by element."""
    g = torch.Generator().manual_seed(parts)
    M, K, N = 40, 640, 96
    h = (torch.randn(M, K, generator=g) * 0.5 + 3.0 * torch.randn(M, 1, generator=g)).half()
    gamma, beta = 1.0 + 0.2 * torch.randn(K, generator=g).double(), 0.3 * torch.randn(K, generator=g).double()
    W, b = torch.randn(N, K, generator=g).double() * K ** -0.5, torch.randn(N, generator=g).double()
    wf = (W * gamma[None, :]).half()                   # the fold as stored; the comparison unfolds it again, exactly
    Wd = wf.double() / gamma[None, :]
    bf = (Wd @ beta + b).half()
    bd = bf.double() - Wd @ beta
    y = F.layer_norm(h.double(), (K,), gamma, beta, FR.LN_EPS) @ Wd.T + bd
    colsum = wf.double().sum(1)
    spec = dict(a=h, w=wf, bias=bf, ln_in=(FR.exact_partials(h, parts), colsum.float(), FR.LN_EPS))
    if geglu:
        spec["epi"] = R.EPI_GEGLU
        val, gate = R.unpair(y)
        y = val * F.gelu(gate)
    p = R.reference("gemm", spec).p
    hd = h.double()
    mean, var = hd.mean(1), hd.var(1, unbiased=False)
    rstd = (var + FR.LN_EPS) ** -0.5
    spread = (hd.reshape(M, parts, -1).mean(-1) - mean[:, None]).abs().amax(1)
    e_mean = 2.0 ** -24 * hd.reshape(M, parts, -1).mean(-1).abs().amax(1)
    e_var = 2.0 ** -23 * var + 2 * spread * 2 * e_mean + 4 * e_mean ** 2
    rel = e_var / (var + FR.LN_EPS)
    lin = (hd - mean[:, None]) @ wf.double().T
    cs_err = (colsum.float().double() - colsum).abs()          # the column sums are handed over as fp32 too
    tol = (rstd * e_mean)[:, None] * colsum.abs()[None, :] + rel[:, None] * (rstd[:, None] * lin).abs() + (rstd * mean.abs())[:, None] * cs_err[None, :] + 1e-12
    if geglu:
        tv, tg = R.unpair(tol)
        v0, g0 = R.unpair(F.layer_norm(hd, (K,), gamma, beta, FR.LN_EPS) @ Wd.T + bd)
        tol = F.gelu(g0).abs() * tv + v0.abs() * 1.13 * tg + 1.13 * tv * tg
    err = (p - y).abs()
    assert bool((err <= tol).all()), float((err / tol).max())
    assert float(err.max()) < 1e-4          # and the tolerance itself is small: the two ARE the same function


@pytest.mark.parametrize("name", LN_IN_NAMES)
def test_ln_in_standin_stays_inside_the_bound(name):
    r = ln_in_ref(name)
    n, worst = R.compare(FR.ln_in_standin(ln_in_all()[name].spec), r.want, r.bound)
    assert n == 0, f"{name}: {n} elements of a correct fp32 kernel outside the bound, worst {worst}"


@pytest.mark.parametrize("mutant", FR.LN_IN_MUTANTS)
@pytest.mark.parametrize("name", LN_IN_NAMES)
def test_ln_in_mutants_leave_the_bound(name, mutant):
    """(With one partial per row [parts][M] and [M][parts] are the same buffer, and with eight the mean IS divided by 8: there the
    two mutants are the correct kernel.)"""
    r = ln_in_ref(name)
    n, _ = R.compare(FR.ln_in_standin(ln_in_all()[name].spec, mutant), r.want, r.bound)
    if (mutant == "index_m_parts" and _parts(name) == 1) or (mutant == "mean_as_8_parts" and _parts(name) == 8):
        assert n == 0, f"{name}: {mutant} is the correct kernel here"
        return
    assert n > 0, f"{name}: the {mutant} mutant passes"


def test_ln_in_cases_reach_every_parts_value_both_signs_and_a_constant_row():
    seen = set()
    for name in LN_IN_NAMES:
        part = ln_in_all()[name].spec["ln_in"][0]
        seen.add(part.shape[0])
        mean, m2 = part[..., 0].double().mean(0), part[..., 1].double().sum(0)
        ratio = mean.abs() / 0.5
        assert bool((mean > 0).any()) and bool((mean < 0).any()), name
        assert bool((ratio > 90).any()) and bool(((ratio > 3) & (ratio < 5)).any()), name
        assert float(m2[FR.ZERO_VAR_ROW]) == 0.0, name
        a = ln_in_all()[name].spec["a"]
        assert a.stride(0) > a.shape[1], "lda > K"
    assert seen == set(FR.LN_PARTS)
    r = ln_in_ref("f16.b.full.p5")
    assert bool(torch.isfinite(r.want[FR.ZERO_VAR_ROW]).all())


# ---- ln_out / gn_out --------------------------------------------------------------------------------------------------------------------
def _producers():
    out = {}
    for form in FORMS:
        for op in ("gemm", "conv", "conv2"):
            if form == "w8" and op != "gemm":
                continue
            for what, c in FR.producer_cases(form, op).items():
                out[f"{form}.{op}.{what}"] = c
    return out


PRODUCERS = _producers()
LN_OUT_NAMES = [n for n in sorted(PRODUCERS) if n.split(".")[1] == "gemm" and n.split(".")[2] in FR.LN_OUT_WHATS]
GN_OUT_NAMES = [n for n in sorted(PRODUCERS) if n.split(".")[2] in FR.GN_OUT_WHATS and not n.startswith("w8")]
BNS = sorted({b.bn for b in FR.BUILDS.values()})
RGS = sorted({FR.gn_layout(b)[2] for b in FR.BUILDS.values()})


@functools.lru_cache(maxsize=None)
def produced(name):
    return FR.producer_standin(PRODUCERS[name])


def _source(name, mutant):
    pre, y1, out = produced(name)
    return {"unrounded": pre, "before_res": y1}.get(mutant, out).numpy()


@pytest.mark.parametrize("bn", BNS)
@pytest.mark.parametrize("name", LN_OUT_NAMES)
def test_ln_out_standin_and_mutants(name, bn):
    """The reference is taken from the stand-in's OWN stored values, as the GPU file takes it from the kernel's.  (`const` has no
    residual: statistics before the residual add are the correct kernel there.)"""
    ref = FR.ln_out_reference(produced(name)[2].double(), bn)
    n, room, worst = FR.stats_compare(FR.ln_out_standin(_source(name, None), bn), ref)
    print(f"{name} BN {bn}: stand-in err / bound {room:.4f}")
    assert n == 0, f"{name}: {n} partials of a correct fp32 kernel outside the bound, {worst}"
    for mutant in FR.STAT_MUTANTS_LN:
        m = mutant if mutant in ("sum_of_squares", "index_m_parts") else None
        n, _, _ = FR.stats_compare(FR.ln_out_standin(_source(name, mutant), bn, m), ref)
        if mutant == "before_res" and name.endswith(".const"):
            assert n == 0, f"{name}: {mutant} is the correct kernel here"
        else:
            assert n > 0, f"{name}: the {mutant} mutant passes"


@pytest.mark.parametrize("rg", RGS)
@pytest.mark.parametrize("name", GN_OUT_NAMES)
def test_gn_out_standin_and_mutants(name, rg):
    """(64 is a multiple of 16 and of 32 row groups: there every group is a full one and `short_group_as_full` is the correct kernel.)"""
    ref = FR.gn_out_reference(produced(name)[2].double(), rg)
    n, room, worst = FR.stats_compare(FR.gn_out_standin(_source(name, None), rg), ref)
    print(f"{name} RG {rg}: stand-in err / bound {room:.4f}")
    assert n == 0, f"{name}: {n} partials of a correct fp32 kernel outside the bound, {worst}"
    for mutant in FR.STAT_MUTANTS_GN:
        m = mutant if mutant not in ("unrounded", "before_res") else None
        n, _, _ = FR.stats_compare(FR.gn_out_standin(_source(name, mutant), rg, m), ref)
        if mutant == "short_group_as_full" and 64 % rg == 0:
            assert n == 0, f"{name}: {mutant} is the correct kernel at RG = {rg}"
        else:
            assert n > 0, f"{name}: the {mutant} mutant passes"


def test_constant_tiles_and_channels_are_exact():
    """A constant row tile (ln_out) and a constant channel (gn_out) come out of the stand-in with the exact mean and M2 = 0: what the
    GPU file asserts of the kernels beside the bound."""
    out = produced("f16.gemm.const")[2]
    for bn in BNS:
        st = FR.ln_out_standin(out.numpy(), bn)[:FR.CONST_COLS // bn]
        assert bool((st[..., 0] == 0.8125).all()) and bool((st[..., 1] == 0).all()), bn
    out = produced("f16.gemm.constch")[2]
    for rg in RGS:
        st = FR.gn_out_standin(out.numpy(), rg)[:, FR.CONST_CH]
        assert bool((st[:, 0] == st[0, 0]).all()) and bool((st[:, 1] == 0).all()), rg
    assert bool((out[:, FR.CONST_CH] == out[0, FR.CONST_CH]).all())


def test_producer_cases_carry_what_their_names_say():
    pre, _, out = produced("f16.gemm.rowmean")
    ratio = out.double().mean(1).abs() / out.double().std(1)
    assert float(ratio.min()) > 80
    out = produced("f16.conv.chanoff")[2].double().reshape(-1, 64, FR.PN)
    ratio = out.mean(1).abs() / out.std(1)
    assert float(ratio.max()) > 80 and bool((out.mean(1) > 0).any()) and bool((out.mean(1) < 0).any())
    assert produced("f16.conv2.rowbias")[2].shape == (512, FR.PN)


# ---- the acceptance tables ----------------------------------------------------------------------------------------------------------------
def test_acceptance_tables_follow_from_the_lds_formulas():
    """The literal lists the GPU probe is held against are what ln_out_fits / gn_out_fits of csrc/gemm_conv.hip give for the builds
    each form has (fp8 weights: the narrower ring, and no gn_out at all; the loader-wave conv exists with the 3-deep ring only)."""
    for form, ids in FR.FORM_IDS.items():
        w8 = form == "w8"
        assert FR.LN_OUT_IDS[form] == [t for t in ids if FR.ln_out_fits(FR.BUILDS[t], w8)], form
        assert FR.GN_OUT_GEMM_IDS[form] == ([] if w8 else [t for t in ids if FR.gn_out_fits(FR.BUILDS[t])]), form
    from golden import make_gemm_conv_bits as maker
    assert FR.GN_OUT_CONV_IDS["f16"] == [t for t in maker.F16_CONV_IDS if FR.gn_out_fits(FR.BUILDS[t])]
    assert FR.GN_OUT_CONV_IDS["bf16"] == [t for t in maker.BF16_IDS if FR.gn_out_fits(FR.BUILDS[t])]
    assert 26 not in FR.LN_OUT_IDS["f16"] and 36 in FR.LN_OUT_IDS["f16"], "256x128: the 3-deep ring has room, the 2-deep one has not"
    assert RGS == [12, 16, 25, 32] and BNS == [64, 128, 160]
