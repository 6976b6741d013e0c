"""CPU: adaptive projected guidance -- the fp64 restatement (tests/apg_ref.py) against itself and against the properties the
contract implies, and the host side: enable_apg's argument ranges, the refused call combinations, the CLI flag, the scalar-row
layout, the ABI table and the entries' argument validation."""
import math

import pytest
import torch

import apg_ref
from instantir_amd.config import UNetConfig

COEF = [6.5, 0.93, 0.37, 0.41, 0.98, 0.12, 0.07, 0.0]
SHAPES = [(2, 4, 5, 7), (1, 4, 48, 40)]


def _case(shape, seed=0):
    """Inputs in the style of tests/test_restore_map_gpu.py::_step_case: eps values of fp16 numbers, x = 3 * randn; image 1's
    cond rows pulled towards its uncond rows so that the images' update norms differ by about 10x."""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(200 + seed + H)
    u = torch.randn(B, C, H, W, generator=g).half().double()
    c = torch.randn(B, C, H, W, generator=g).half().double()
    if B > 1:
        c[1] = (u[1] + 0.1 * (c[1] - u[1])).half().double()
    x = (torch.randn(B, C, H, W, generator=g) * 3).double()
    a_prev = (torch.randn(B, C, H, W, generator=g) * 2).double()
    return u, c, x, a_prev


def _dot(a, b):
    return (a * b).sum(dim=(1, 2, 3))


@pytest.mark.parametrize("shape", SHAPES)
def test_identity_parameters_reproduce_plain_cfg(shape):
    u, c, x, a_prev = _case(shape)
    eps, A, s, alpha = apg_ref.apg_eps(u, c, x, a_prev, COEF, eta=1.0, r=0.0, beta=0.0)
    want = apg_ref.cfg_eps(u, c, COEF[0])
    rel = ((eps - want).abs().max() / want.abs().max()).item()
    print(f"{shape}: identity parameters vs u + w (c - u): max abs {(eps - want).abs().max().item():.2e}, relative {rel:.2e}")
    assert rel <= 1e-12
    assert torch.equal(s, torch.ones_like(s))


@pytest.mark.parametrize("shape", SHAPES)
def test_eta_zero_leaves_no_parallel_part(shape):
    u, c, x, a_prev = _case(shape)
    sb, sa = [float(torch.tensor(v, dtype=torch.float32)) for v in COEF[1:3]]
    for r, beta in ((0.0, 0.0), (7.0, -0.5)):
        eps, A, s, alpha = apg_ref.apg_eps(u, c, x, a_prev, COEF, eta=0.0, r=r, beta=beta)
        x0c = (x - sb * c) / sa
        x0g = (x - sb * eps) / sa
        cos = _dot(x0g - x0c, x0c) / (_dot(x0g - x0c, x0g - x0c).sqrt() * _dot(x0c, x0c).sqrt())
        assert cos.abs().max().item() <= 1e-12, cos


def test_norm_clamp():
    u, c, x, a_prev = _case(SHAPES[0])
    _, A, s, _ = apg_ref.apg_eps(u, c, x, a_prev, COEF, eta=0.0, r=0.0, beta=0.0)
    n = _dot(A, A).sqrt()
    r = float(torch.tensor(0.5 * n[0].item(), dtype=torch.float32))
    _, A, s, _ = apg_ref.apg_eps(u, c, x, a_prev, COEF, eta=0.0, r=r, beta=0.0)
    assert s[0] < 1 and s[1] == 1.0                         # clamp active for image 0, inactive (exactly 1) for image 1
    assert abs((s[0] * n[0]).item() - r) <= 1e-12 * r       # ||s A|| == r
    _, _, s0, _ = apg_ref.apg_eps(u, c, x, a_prev, COEF, eta=0.0, r=0.0, beta=0.0)
    assert torch.equal(s0, torch.ones(2, dtype=torch.float64))     # r == 0: no clamp


def test_momentum_recurrence_over_three_steps():
    shape = SHAPES[0]
    sb, sa = [float(torch.tensor(v, dtype=torch.float32)) for v in COEF[1:3]]
    beta = -0.5
    steps = [_case(shape, seed=k) for k in range(3)]
    A = torch.full(shape, float("nan"), dtype=torch.float64)      # never read on the first step
    got = []
    for k, (u, c, x, _) in enumerate(steps):
        _, A, _, _ = apg_ref.apg_eps(u, c, x, A, COEF, eta=0.0, r=0.0, beta=0.0 if k == 0 else beta)
        got.append(A)
    D = [((x - sb * c) / sa) - ((x - sb * u) / sa) for (u, c, x, _) in steps]
    want = [D[0], D[1] + beta * D[0], D[2] + beta * (D[1] + beta * D[0])]
    for a, b in zip(got, want):
        assert torch.isfinite(a).all() and (a - b).abs().max().item() <= 1e-13 * b.abs().max().item()


def test_images_are_independent():
    u, c, x, a_prev = _case(SHAPES[0])
    base = apg_ref.apg_eps(u, c, x, a_prev, COEF, eta=0.25, r=9.0, beta=-0.5)
    u2, c2, x2, a2 = (v.clone() for v in (u, c, x, a_prev))
    for v in (u2, c2, x2, a2):
        v[1] = v[1] * 1.7 + 0.3
    other = apg_ref.apg_eps(u2, c2, x2, a2, COEF, eta=0.25, r=9.0, beta=-0.5)
    for a, b in zip(base, other):
        assert torch.equal(a[0], b[0]) and not torch.equal(a[1], b[1])


def test_fp32_restatement_is_close_to_fp64():
    u, c, x, a_prev = _case(SHAPES[1])
    e64 = apg_ref.apg_eps(u, c, x, a_prev, COEF, eta=0.0, r=100.0, beta=-0.5)
    e32 = apg_ref.apg_eps(u, c, x, a_prev, COEF, eta=0.0, r=100.0, beta=-0.5, fp32=True)
    err = (e32[0] - e64[0]).abs().max().item()
    print(f"fp32 restatement: max |fp32 - fp64| = {err:.2e} on |eps| up to {e64[0].abs().max().item():.1f}")
    assert 0 < err <= 64 * 2.0 ** -24 * e64[0].abs().max().item()


# ---- host side ------------------------------------------------------------------------------------------------------------------
def _pipe():
    from instantir_amd.pipeline import InstantIRPipeline
    return InstantIRPipeline(UNetConfig.tiny(), {}, device="cpu")


def test_enable_disable_and_defaults():
    p = _pipe()
    assert p.apg is None
    p.enable_apg()
    assert p.apg == (0.0, 15.0, -0.5)
    p.enable_apg(eta=1, norm_threshold=0, momentum=0.9)
    assert p.apg == (1.0, 0.0, 0.9)
    p.disable_apg()
    assert p.apg is None
    with pytest.raises(AttributeError):
        p.apg = (0.0, 1.0, 0.0)                                   # read-only


@pytest.mark.parametrize("kw", [dict(eta=-0.01), dict(eta=1.01), dict(eta=math.nan), dict(norm_threshold=-1.0),
                                dict(norm_threshold=math.inf), dict(momentum=1.0), dict(momentum=-1.0), dict(momentum=math.nan),
                                dict(eta="x"), dict(momentum=None)])
def test_enable_apg_argument_ranges(kw):
    p = _pipe()
    p.enable_apg(0.5, 3.0, 0.25)
    with pytest.raises(ValueError, match="enable_apg"):
        p.enable_apg(**kw)
    assert p.apg == (0.5, 3.0, 0.25)                              # a refused change leaves the setting as it was


def _call(p, **kw):
    return p(image=torch.zeros(1, 4, 8, 8), prompt_embeds=torch.zeros(1, 77, 64), pooled_prompt_embeds=torch.zeros(1, 32), **kw)


@pytest.mark.parametrize("g", [1.0, 0.0])
def test_apg_refuses_a_call_without_guidance(g):
    p = _pipe()
    p.enable_apg()
    with pytest.raises(ValueError, match="guidance_scale"):
        _call(p, guidance_scale=g)


def test_apg_refuses_guidance_rescale():
    p = _pipe()
    p.enable_apg()
    with pytest.raises(ValueError, match=r"(?s)guidance_rescale.*enable_apg"):
        _call(p, guidance_scale=7.0, guidance_rescale=0.7)


def test_cli_apg_flag():
    from instantir_amd.infer import apply_apg, build_parser
    bp = build_parser()
    a = bp.parse_args(["--test_path", "x"])
    assert a.apg is None
    p = _pipe()
    apply_apg(p, a)
    assert p.apg is None                                          # default: the pipeline stays as built
    a = bp.parse_args(["--test_path", "x", "--apg", "0.25", "12", "-0.5"])
    assert a.apg == [0.25, 12.0, -0.5]
    apply_apg(p, a)
    assert p.apg == (0.25, 12.0, -0.5)
    with pytest.raises(SystemExit):
        bp.parse_args(["--test_path", "x", "--apg", "0.25", "12"])
    with pytest.raises(ValueError, match="eta"):
        apply_apg(_pipe(), bp.parse_args(["--test_path", "x", "--apg", "2", "12", "0"]))


@pytest.mark.parametrize("rows", [2, 3, 6])
def test_scalar_row_gains_the_apg_group_last(rows):
    from instantir_amd.pipeline import _scalar_row
    names = ["t", "lcm", "sched", "res_scale", "c_in", "pag_s"]
    plain, n = _scalar_row(rows)
    assert list(plain) == names and n == 2 * rows + 14
    masked, nm = _scalar_row(rows, True)
    assert list(masked) == names + ["keep"] and nm == n + 4 and all(masked[k] == plain[k] for k in plain)
    for m, base, nb in ((False, plain, n), (True, masked, nm)):
        lay, na = _scalar_row(rows, m, True)
        assert list(lay) == list(base) + ["apg"] and lay["apg"] == slice(nb, nb + 4) and na == nb + 4
        assert all(lay[k] == base[k] for k in base)


def test_abi_table_has_both_entries():
    from instantir_amd import lib
    import ctypes
    assert "iir_apg_project" in lib.SIGNATURES and "iir_sched_step" in lib.SIGNATURES
    fields = [name for name, _ in lib.SchedDesc._fields_]
    assert len(lib.SIGNATURES["iir_apg_project"][1]) == 13 and all(k in fields for k in ("apg_avg", "apg_sa", "apg_par"))
    declared = lib.declared_symbols()
    assert "iir_apg_project" in declared and "iir_sched_step" in declared
    h = ctypes.CDLL(lib.LIB_PATH)
    assert hasattr(h, "iir_apg_project") and hasattr(h, "iir_sched_step")


def test_apg_entries_reject_bad_arguments_without_a_gpu():
    import ctypes
    from instantir_amd import lib
    h = lib.load()
    assert h.iir_abi_version() == 3
    P = 4096

    need = h.iir_apg_project_workspace_bytes(1)
    assert need > 0 and h.iir_apg_project_workspace_bytes(8) == 8 * need and h.iir_apg_project_workspace_bytes(0) == 0

    def proj(**kw):
        a = dict(eps=P, lde=8, B=1, C=4, HW=64, coef=P, x=P + 1024, par=P, avg=P + 2048, sa=P + 4096, ws=P + 8192, nws=need)
        a.update(kw)
        return h.iir_apg_project(a["eps"], a["lde"], a["B"], a["C"], a["HW"], a["coef"], a["x"], a["par"], a["avg"], a["sa"], a["ws"],
                                 a["nws"], None)

    for k in ("eps", "coef", "x", "par", "avg", "sa", "ws"):
        assert proj(**{k: None}) == -1, k
    assert proj(B=0) == -1 and proj(C=0) == -1 and proj(HW=0) == -1 and proj(B=-1) == -1 and proj(lde=3) == -1
    assert proj(avg=P + 1024) == -1                               # the average may not be x
    assert proj(nws=need - 1) == -1 and proj(ws=P + 8196) == -1 and proj(B=2) == -1      # workspace too small / unaligned

    def step(**kw):
        a = dict(eps_nhwc=P, lde=8, B=1, C=4, HW=64, cfg=1, coef=P, x=P + 1024, prev=P + 2048, apg_avg=P + 4096, apg_sa=P + 8192,
                 apg_par=P)
        a.update(kw)
        # what iir_sched_step_apg implied: the APG bit, and the bit of every optional group with a pointer given
        a.setdefault("groups", lib.STEP_APG | (lib.STEP_HIST if a.get("hist") else 0)
                     | (lib.STEP_KEEP if any(a.get("keep_" + k) for k in ("map", "src", "noise", "coef")) else 0))
        return h.iir_sched_step(ctypes.byref(lib.SchedDesc(**a)), None)

    for k in ("eps_nhwc", "coef", "x", "prev", "apg_avg", "apg_sa", "apg_par"):
        assert step(**{k: None}) == -1, k
    assert step(B=0) == -1 and step(C=0) == -1 and step(HW=0) == -1 and step(lde=3) == -1
    assert step(cfg=0) == -1                                      # nothing to project without the uncond rows
    assert step(keep_map=P) == -1 and step(keep_map=P, keep_src=P, keep_noise=P) == -1      # the keep group: all four pointers or none
    assert step(hist=P + 16384, eps_out=P + 32768) == -1          # eps_out together with hist
    assert step(apg_avg=P + 2048) == -1                           # the average may not be an output plane
    assert step(hist=P + 1024) == -1                              # hist aliases x
    assert step(groups=0) == -1 and step(apg_avg=None, apg_sa=None, groups=0) == -1      # pointers without the bit
    assert step(keep_map=P, groups=lib.STEP_APG) == -1 and step(groups=lib.STEP_APG | 64) == -1      # ... and a bit outside the four
