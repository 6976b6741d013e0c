"""CPU: the fp64 reference and error bound of tests/gemm_conv_ref.py, checked without a GPU.

The reference's convolution equals torch's in float64 for every geometry the GPU file launches; its paired epilogues equal the
un-permuted formulas; an fp32 stand-in kernel (torch.matmul / conv2d in fp32, then the two roundings) stays inside the bound with
0 elements out at every shape the GPU file runs; and each wrong kernel one could plausibly write (the mutants) leaves it."""
import functools

import pytest
import torch
import torch.nn.functional as F

import gemm_conv_ref as R


@functools.lru_cache(maxsize=None)
def all_cases():
    out = {}
    for form in ("f16", "bf16", "w8", "f8"):
        for n, c in R.gemm_cases(form).items():
            out[f"gemm.{form}.{n}"] = c
        for n, c in R.act_cases(form).items():
            out[f"act.{form}.{n}"] = c
    for form in ("f16", "f8"):
        for n, c in R.gemm8_cases(form).items():
            out[f"gemm.{form}.{n}"] = c
    for form in ("f16", "bf16"):
        for n, c in R.conv_cases(form).items():
            out[f"conv.{form}.{n}"] = c
    out["conv.f16.sft"] = R.sft_case()
    out["gemm.f16.big64"], out["gemm.f16.big128"] = R.big_case(), R.big_case(128)
    return out


@functools.lru_cache(maxsize=None)
def ref_of(name):
    return R.reference(*all_cases()[name])


NAMES = sorted(all_cases())
CONV_NAMES = [n for n in NAMES if all_cases()[n].kind == "conv"]


def _is(name, **want):
    """Does the case's spec hold these values (missing keys count as the wrapper's defaults)?"""
    s = all_cases()[name].spec
    dflt = dict(epi=R.EPI_PLAIN, act=R.ACT_NONE, pad_mode=0, ksize=3)
    return all(s.get(k, dflt.get(k)) == v for k, v in want.items())


def _conv32(s, mutant):
    """fp32 F.conv2d of a conv spec -> (M, Cout).  Mutants: swap_hw (the gather takes H for W), pad_neighbour (one padding pixel,
    above the first pixel of every image -- below it for pad_mode = 1 -- reads that pixel and not zero), pad1_symmetric (pad_mode = 1 taken for symmetric)."""
    x, w = s["x"], s["w"]
    ks, stride, ups, pad_mode = s.get("ksize", 3), s.get("stride", 1), s.get("upsample", False), s.get("pad_mode", 0)
    xs = x.float().contiguous()
    if mutant == "swap_hw":
        xs = xs.reshape(x.shape[0], x.shape[2], x.shape[1], x.shape[3])
    xn = xs.permute(0, 3, 1, 2)
    if ups:
        xn = F.interpolate(xn, scale_factor=2.0, mode="nearest")
    if pad_mode == 1 and mutant != "pad1_symmetric":
        xn = F.pad(xn, (0, 1, 0, 1))
    else:
        xn = F.pad(xn, (ks // 2,) * 4)
    if mutant == "pad_neighbour":
        xn = xn.clone()
        if pad_mode == 1:
            xn[:, :, -1, 1] = xn[:, :, -2, 1]
        else:
            xn[:, :, 0, 1] = xn[:, :, 1, 1]
    y = F.conv2d(xn, w.float().permute(0, 3, 1, 2).contiguous(), stride=stride)
    if mutant == "pad1_symmetric":
        Ho, Wo = R.conv_out_size(x.shape[1], x.shape[2], ks, stride, ups, 1)
        y = y[:, :, :Ho, :Wo]
    return y.permute(0, 2, 3, 1).reshape(-1, w.shape[0])


def standin(name, mutant=None):
    """A correct kernel in fp32: torch.matmul / conv2d, the epilogue in fp32, the two roundings.  `mutant` breaks it."""
    kind, s = all_cases()[name]
    s = dict(s)
    dt = ref_of(name).dtype if ref_of(name).dtype != torch.float32 else s["a"].dtype
    epi, act, out_scale = s.get("epi", R.EPI_PLAIN), s.get("act", R.ACT_NONE), s.get("out_scale", 1.0)
    scale = None
    if kind == "conv":
        if mutant == "drop_k":
            s["w"] = s["w"].clone()
            s["w"][:, -1, -1, -1] = 0
        v = _conv32(s, mutant)
        Ho, Wo = R.conv_out_size(s["x"].shape[1], s["x"].shape[2], s.get("ksize", 3), s.get("stride", 1), s.get("upsample", False), s.get("pad_mode", 0))
        hw = Ho * Wo
    else:
        hw = 1
        if kind == "gemm_fp8":
            a, (w, scale) = s["a8"].float(), s["w8"]
            scale = scale * s["a_scale"]
        else:
            a, w, scale = s["a"].float(), s["w"], s.get("wscale")
            if scale is not None:
                a = R.to_e4m3(s["a"]).float()
        w = w.float().clone()
        if mutant == "drop_k":
            w[:, -1] = 0
        v = a @ w.T
    if scale is not None:
        v = v * scale[None, :]
    M = v.shape[0]
    bias = s["bias"].float()[None, :] if s.get("bias") is not None else 0.0
    if mutant != "bias_after_act":
        v = v + bias
    if s.get("rowbias") is not None:
        v = v + s["rowbias"].float()[torch.arange(M) // s["rows_per_rb"]]
    res = s["res"].float()[R.image_rows(M, hw, s.get("res_img_rows", 0))] if s.get("res") is not None else None
    if epi == R.EPI_PLAIN:
        v = {R.ACT_NONE: lambda t: t, R.ACT_SILU: F.silu, R.ACT_GELU: F.gelu, R.ACT_QUICKGELU: lambda t: t * torch.sigmoid(1.702 * t)}[act](v)
        if mutant == "bias_after_act":
            v = v + bias
        if s.get("out_dtype") == torch.float32:
            out = v * out_scale
        elif mutant == "res_before_round":
            out = ((v + res) * out_scale).to(dt)
        else:
            y1 = v.to(dt).float()
            out = ((y1 + res if res is not None else y1) * out_scale).to(dt)
    else:
        val, par = R.unpair(v)
        out = ((val * F.gelu(par) if epi == R.EPI_GEGLU else res * (val + 1.0) + par).to(dt).float() * out_scale).to(dt)
    out = out.double()
    if mutant == "swap_rows":
        out[[5, 6]] = out[[6, 5]]
    return out


# ---- the reference against torch in float64 ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CONV_NAMES)
def test_reference_conv_equals_torch_fp64(name):
    """im2col(x) @ W^T, gathered from the input's storage by its pixel and image strides, is F.conv2d in float64 (of
    F.interpolate(nearest, 2x) for the upsample, of F.pad(x, (0, 1, 0, 1)) for pad_mode = 1), to 1e-12."""
    s = all_cases()[name].spec
    x, w = s["x"], s["w"]
    ks, stride, ups, pad_mode = s["ksize"], s["stride"], s["upsample"], s["pad_mode"]
    assert x.stride(2) > x.shape[3], "the pixel stride must exceed Cin"
    xn = x.double().permute(0, 3, 1, 2)
    if ups:
        xn = F.interpolate(xn, scale_factor=2.0, mode="nearest")
    xn = F.pad(xn, (0, 1, 0, 1)) if pad_mode == 1 else F.pad(xn, (ks // 2,) * 4)
    want = F.conv2d(xn, w.double().permute(0, 3, 1, 2), stride=stride)
    assert tuple(want.shape[2:]) == R.conv_out_size(x.shape[1], x.shape[2], ks, stride, ups, pad_mode)
    got = R.im2col(x, ks, stride, ups, pad_mode) @ w.double().reshape(w.shape[0], -1).T
    assert (got - want.permute(0, 2, 3, 1).reshape(got.shape)).abs().max().item() <= 1e-12


def test_reference_conv_geometries_cover_the_free_strides():
    c = all_cases()
    assert c["conv.f16.a"].spec["x"].shape[1] != c["conv.f16.a"].spec["x"].shape[2], "non-square"
    x = c["conv.f16.f"].spec["x"]
    assert x.stride(0) > x.shape[1] * x.stride(1) and x.stride(2) > x.shape[3], "padded image stride and pixel stride"


def test_reference_paired_epilogues_equal_the_unpermuted_formulas():
    """GEGLU and SFT on the `pair_rows` layout are h[:, :n] * gelu(h[:, n:]) and h * (gamma + 1) + beta of the un-permuted weights:
    the formulas of test_gemm_geglu / test_conv_sft_epilogue, in float64."""
    from instantir_amd.packing import pair_rows
    g = torch.Generator().manual_seed(3)
    M, n, K = 50, 48, 64
    a, w, b = (torch.randn(M, K, generator=g).half(), (torch.randn(2 * n, K, generator=g) / 8).half(), torch.randn(2 * n, generator=g).half())
    h = a.double() @ w.double().T + b.double()
    r = R.reference("gemm", dict(a=a, w=pair_rows(w[:n], w[n:]), bias=pair_rows(b[:n], b[n:]), epi=R.EPI_GEGLU))
    assert (r.p - h[:, :n] * F.gelu(h[:, n:])).abs().max().item() <= 1e-12
    Rn, H, W, Ch, C = 2, 5, 6, 64, 48
    actv, hh = torch.randn(Rn, H, W, Ch, generator=g).half(), torch.randn(Rn * H * W, C, generator=g).half()
    wm, wa = ((torch.randn(C, 3, 3, Ch, generator=g) / 24).half() for _ in range(2))
    bm, ba = torch.randn(C, generator=g).half(), torch.randn(C, generator=g).half()
    conv = lambda wt, bt: F.conv2d(actv.double().permute(0, 3, 1, 2), wt.double().permute(0, 3, 1, 2), bt.double(), padding=1).permute(0, 2, 3, 1).reshape(-1, C)
    r = R.reference("conv", dict(x=actv, w=pair_rows(wm, wa), bias=pair_rows(bm, ba), res=hh, epi=R.EPI_SFT))
    assert (r.p - (hh.double() * (conv(wm, bm) + 1) + conv(wa, ba))).abs().max().item() <= 1e-12


def test_rounding_and_compare_helpers():
    x = torch.tensor([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 65504.0, 2.0 ** -25 * 1.01], dtype=torch.float64)
    assert R.round_e(x, torch.float16).tolist() == [1.0, 1.0 + 2.0 ** -9, 65504.0, 2.0 ** -24]          # ties to even, subnormal step
    assert R.round_e(torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8], dtype=torch.float64), torch.bfloat16).tolist() == [1.0, 1.0 + 2.0 ** -6]
    want, bound = torch.zeros(2, 3, dtype=torch.float64), torch.full((2, 3), 0.5, dtype=torch.float64)
    got = want.clone()
    assert R.compare(got, want, bound) == (0, None)
    got[1, 2], got[0, 1] = 2.0, float("nan")
    n, worst = R.compare(got, want, bound)
    assert n == 2 and worst["index"] == (0, 1)


# ---- the bound: the reference model stays inside it, wrong kernels do not ----------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_standin_kernel_stays_inside_the_bound(name):
    r = ref_of(name)
    n, worst = R.compare(standin(name), r.want, r.bound)
    assert n == 0, f"{name}: {n} elements of a correct fp32 kernel outside the bound, worst {worst}"


def test_first_order_form_is_no_bound():
    """Why the bound is the interval image and not u |p| + u |want| + d + tiny: the correct stand-in breaks that form where a
    rounding tie lies between p and the fp32 value and the residual cancels (see the module docstring of gemm_conv_ref)."""
    r = ref_of("gemm.f16.big64")
    n, _ = R.compare(standin("gemm.f16.big64"), r.want, r.first_order)
    print(f"stand-in elements outside the first-order form at 512 x 640 x 64: {n}")
    assert n > 0


@pytest.mark.parametrize("mutant", ["drop_k", "swap_rows"])
@pytest.mark.parametrize("name", NAMES)
def test_mutants_of_every_shape_leave_the_bound(name, mutant):
    """One K element dropped (the last column of the last K tile); two adjacent output rows swapped inside one tile."""
    r = ref_of(name)
    n, _ = R.compare(standin(name, mutant), r.want, r.bound)
    assert n > 0, f"{name}: the {mutant} mutant passes"


@pytest.mark.parametrize("name", [n for n in NAMES if _is(n, epi=R.EPI_PLAIN) and not _is(n, act=R.ACT_NONE)])
def test_bias_after_the_activation_leaves_the_bound(name):
    r = ref_of(name)
    n, _ = R.compare(standin(name, "bias_after_act"), r.want, r.bound)
    assert n > 0, name


RES_BEFORE_ROUND_MIN = 3


@pytest.mark.parametrize("name", [n for n in NAMES if _is(n, epi=R.EPI_PLAIN) and all_cases()[n].spec.get("res") is not None])
def test_residual_before_the_first_rounding_leaves_the_bound(name):
    """Rounding (p + res) * out_scale once differs from the documented order only where the first rounding error survives the second:
    a few elements per launch.  The seeded inputs give between RES_BEFORE_ROUND_MIN and a few thousand per shape (printed)."""
    r = ref_of(name)
    n, _ = R.compare(standin(name, "res_before_round"), r.want, r.bound)
    print(f"{name}: {n} of {r.want.numel()} elements show a residual added before the first rounding")
    assert n >= RES_BEFORE_ROUND_MIN, name


@pytest.mark.parametrize("name", [n for n in CONV_NAMES if not _is(n, ksize=1)])
@pytest.mark.parametrize("mutant", ["swap_hw", "pad_neighbour"])
def test_conv_gather_mutants_leave_the_bound(name, mutant):
    """H and W exchanged in the gather; one padding pixel read as its neighbour.  (A 1 x 1 conv has neither padding nor a
    neighbourhood: its gather is the identity on pixels, so those shapes have no such mutant.  pad_mode = 1 on the odd 11 x 15 map
    reads no padding pixel at all, so there the second mutant is the correct kernel; so is the first on the square 16 x 16 map.)"""
    x = all_cases()[name].spec["x"]
    if (mutant == "pad_neighbour" and name.endswith(".c1")) or (mutant == "swap_hw" and x.shape[1] == x.shape[2]):
        r = ref_of(name)
        assert R.compare(standin(name, mutant), r.want, r.bound)[0] == 0
        return
    r = ref_of(name)
    n, _ = R.compare(standin(name, mutant), r.want, r.bound)
    assert n > 0, f"{name}: the {mutant} mutant passes"


@pytest.mark.parametrize("name", [n for n in CONV_NAMES if _is(n, pad_mode=1)])
def test_pad_mode_1_taken_for_symmetric_leaves_the_bound(name):
    r = ref_of(name)
    n, _ = R.compare(standin(name, "pad1_symmetric"), r.want, r.bound)
    assert n > 0, name
