"""GPU: adaptive projected guidance (APG) -- iir_apg_project and iir_sched_step_apg through `ops` against the fp64 restatement
of tests/apg_ref.py, their bit properties, and the denoising loop against an APG'd fp32 CPU oracle.

The oracle loops (oracle.pipeline.denoise, the sigma-scheduler loop of tests/loop_ref.py) get APG through their `guide` hook:
loop_ref.apg, the guided eps of `apg_ref.apg_eps` with its running average.

Kernel tolerance (measured in the test, printed before it is asserted): the kernel's max |value - fp64| may be at most 4x the
fp32 restatement's own max |fp32 - fp64| on the same inputs -- 4 covers fma contraction and a different but fixed summation
order.  {s, alpha} are accumulated in fp64 and held to 1e-6 relative."""
import functools

import numpy as np
import pytest
import torch

import apg_ref
import loop_ref as lr
from loop_ref import dev, env  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

C, LDE = 4, 8
# (B, H, W); the reduction gives each of its 32 workgroups per image a run of ceil(HW / 32) pixels, 256 threads wide: HW = 35 leaves
# runs of 2 pixels and 14 empty workgroups, 1920 runs of 60 (less than one pass), 9600 runs of 300 (a second, partial pass of the
# strided loop), 16384 -- the real latent plane, three images -- runs of 512 (two full passes)
SHAPES = [(2, 5, 7), (1, 48, 40), (3, 128, 128), (1, 96, 100)]
ETA, BETA = 0.0, -0.5


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def _coef(form):
    return [6.5, 0.93, 0.37, 0.41, 0.98, 0.12, 0.07, -0.031 if form == "hist" else 0.0]


_CASES = {}


def _case(shape, seed=0):
    """CPU tensors in the style of tests/test_restore_map_gpu.py::_step_case; image 1's cond rows are pulled to u + 0.1 (c - u),
    so that the images' update norms differ by about 10x, and r is half of image 0's norm: both sides of the clamp."""
    key = (shape, seed)
    if key not in _CASES:
        B, H, W = shape
        HW = H * W
        g = torch.Generator().manual_seed(300 + seed + H)
        eps = torch.randn(2 * B * HW, LDE, generator=g).half()
        if B > 1:
            e = eps.view(2, B, HW, LDE)
            e[1, 1] = (e[0, 1].float() + 0.1 * (e[1, 1].float() - e[0, 1].float())).half()
        t = dict(eps=eps, x=torch.randn(B, C, H, W, generator=g) * 3, noise=torch.randn(B, C, H, W, generator=g),
                 hist=torch.randn(B, C, H, W, generator=g), a_prev=torch.randn(B, C, H, W, generator=g) * 2)
        e64 = apg_ref.unpack_eps(eps, 2 * B, C, H, W)
        t["u"], t["c"] = e64[:B], e64[B:]
        _, A, _, _ = apg_ref.apg_eps(t["u"], t["c"], t["x"], t["a_prev"], _coef("linear"), ETA, 0.0, BETA)
        t["r"] = float(torch.tensor(0.5 * A[0].pow(2).sum().sqrt().item(), dtype=torch.float32))
        _CASES[key] = t
    return _CASES[key]


_REFS = {}


def _ref(shape, form, fp32, seed=0):
    """(eps, A, s, alpha, prev, x0) of the case, fp64 or the fp32 restatement; computed once."""
    key = (shape, form, fp32, seed)
    if key not in _REFS:
        t = _case(shape, seed)
        coef = _coef(form)
        eps, A, s, alpha = apg_ref.apg_eps(t["u"], t["c"], t["x"], t["a_prev"], coef, ETA, t["r"], BETA, fp32=fp32)
        prev, x0 = apg_ref.step(eps, t["x"], coef, t["hist"] if form == "hist" else None, t["noise"], fp32=fp32)
        _REFS[key] = (eps, A, s, alpha, prev, x0)
    return _REFS[key]


def _par(dev, eta, r, beta):
    return torch.tensor([eta, r, beta, 0.0], dtype=torch.float32, device=dev)


def _launch(dev, t, form, par, *, a_prev=None, eps=None, x=None, use_hist=None, keep=None, pag=None, want_eps=None):
    """iir_apg_project, then iir_sched_step_apg -> dict(prev, x0, hist, eps_out, A, sa).  `use_hist`: pass the history plane
    (default: in the hist form); eps_out is returned when no history plane is passed."""
    from instantir_amd import ops
    B = t["x"].shape[0]
    use_hist = (form == "hist") if use_hist is None else use_hist
    want_eps = (not use_hist) if want_eps is None else want_eps
    eps = (t["eps"] if eps is None else eps).to(dev)
    x = (t["x"] if x is None else x).to(dev)
    A = (t["a_prev"] if a_prev is None else a_prev).clone().to(dev)
    sa = torch.full((2 * B,), 7.0, device=dev)
    coef = torch.tensor(_coef(form), device=dev)
    prev, x0 = torch.full_like(x, 7.0), torch.full_like(x, 7.0)
    hist = t["hist"].clone().to(dev) if use_hist else None
    eps_out = torch.full_like(x, 7.0) if want_eps else None
    ops.apg_project(eps, B, coef, x, (A, sa, par), ops.apg_workspace(B, dev))
    ops.sched_step(eps, B, coef, x, prev, noise=t["noise"].to(dev), cfg=True, x0_out=x0, eps_out=eps_out, pag_scale=pag, hist=hist,
                   keep=keep, apg=(A, sa, par))
    torch.cuda.synchronize()
    return dict(prev=prev, x0=x0, hist=hist, eps_out=eps_out, A=A, sa=sa)


def _err(a, b):
    return (a.detach().cpu().double() - b.double()).abs().max().item()


# ---- kernels against fp64 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["linear", "hist"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernels_match_fp64(dev, shape, form):
    t = _case(shape)
    B = shape[0]
    eps64, A64, s64, al64, prev64, x064 = _ref(shape, form, False)
    eps32, A32, s32, al32, prev32, x032 = _ref(shape, form, True)
    # both sides of the clamp are exercised, on the fp64 reference alone
    assert s64[0] < 1
    if B > 1:
        assert s64[1] == 1.0
    par = _par(dev, ETA, t["r"], BETA)
    out = _launch(dev, t, form, par)                                  # the form's launch (history plane in the hist form)
    eo = _launch(dev, t, form, par, use_hist=False)                   # eps_out does not combine with a history plane
    sa = out["sa"].cpu().double().view(B, 2)
    rel_s = ((sa[:, 0] - s64).abs() / s64.abs()).max().item()
    rel_a = ((sa[:, 1] - al64).abs() / al64.abs()).max().item()
    print(f"apg {shape} {form}: s = {[round(v, 4) for v in s64.tolist()]}, {{s, alpha}} relative error {rel_s:.2e} / {rel_a:.2e}")
    rows = (("eps", eo["eps_out"], eps64, eps32), ("A", out["A"], A64, A32), ("prev", out["prev"], prev64, prev32),
            ("x0", out["x0"], x064, x032))
    bad = []
    for name, got, w64, w32 in rows:
        e_k, e_32 = _err(got, w64), (w32 - w64).abs().max().item()
        print(f"apg {shape} {form}: {name}: kernel max|. - fp64| = {e_k:.3e}, fp32 restatement {e_32:.3e} (ratio {e_k / e_32:.2f}), "
              f"max|{name}| = {w64.abs().max().item():.1f}")
        if not e_k <= 4 * e_32:
            bad.append((name, e_k, e_32))
    assert rel_s <= 1e-6 and rel_a <= 1e-6
    assert not bad, bad
    assert same_bits(out["A"], eo["A"]) and same_bits(out["sa"], eo["sa"])
    if form == "hist":
        assert same_bits(out["hist"], out["x0"])


# ---- bit properties -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_two_launches_give_equal_bits(dev, shape):
    t = _case(shape)
    par = _par(dev, ETA, t["r"], BETA)
    a, b = _launch(dev, t, "hist", par), _launch(dev, t, "hist", par)
    for k in ("prev", "x0", "hist", "A", "sa"):
        assert same_bits(a[k], b[k]), k


_NAN16 = [0x7E00, 0x7C01, 0xFE00, 0x7C00]                                 # quiet / signalling NaN and Inf bit patterns
_NAN32 = [0x7FC00000, 0x7F800001, -4194304, 0x7F800000, -8388608]        # ... as int32: 0xFFC00000 (-NaN), 0xFF800000 (-Inf)


@pytest.mark.parametrize("shape", SHAPES[:2], ids=lambda s: "x".join(map(str, s)))
def test_beta_zero_never_loads_the_average(dev, shape):
    t = _case(shape)
    par = _par(dev, ETA, t["r"], 0.0)
    pat = torch.tensor(_NAN32, dtype=torch.int32).view(torch.float32)
    poison = pat[torch.arange(t["x"].numel()) % len(_NAN32)].view_as(t["x"])
    for form in ("linear", "hist"):
        clean = _launch(dev, t, form, par, a_prev=torch.zeros_like(t["x"]), want_eps=False)
        got = _launch(dev, t, form, par, a_prev=poison, want_eps=False)
        for k in ("prev", "x0", "A", "sa"):
            assert torch.isfinite(got[k]).all() and same_bits(got[k], clean[k]), (form, k)


def test_nan_in_pad_columns_and_perturbed_rows_stays_out(dev):
    shape = SHAPES[0]
    t = _case(shape)
    B, H, W = shape
    HW = H * W
    par = _par(dev, ETA, t["r"], BETA)
    clean = _launch(dev, t, "hist", par)
    nan16 = torch.tensor(_NAN16, dtype=torch.int32).to(torch.int16).view(torch.float16)
    eps = torch.empty(3 * B * HW, LDE, dtype=torch.float16)
    eps[:2 * B * HW] = t["eps"]
    eps[:, C:] = nan16[torch.arange(LDE - C) % 4]                      # pad columns of every row
    eps[2 * B * HW:] = nan16[torch.arange(LDE) % 4]                    # the perturbed rows, whole
    got = _launch(dev, t, "hist", par, eps=eps, pag=torch.zeros(1, device=dev))
    for k in ("prev", "x0", "hist", "A", "sa"):
        assert torch.isfinite(got[k]).all() and same_bits(got[k], clean[k]), k


def test_images_are_independent(dev):
    shape = SHAPES[0]
    t = _case(shape)
    B, H, W = shape
    HW = H * W
    par = _par(dev, 0.25, t["r"], BETA)
    base = _launch(dev, t, "linear", par)
    g = torch.Generator().manual_seed(9)
    eps = t["eps"].clone().view(2, B, HW, LDE)
    eps[:, 1] = torch.randn(2, HW, LDE, generator=g).half()
    x, a_prev = t["x"].clone(), t["a_prev"].clone()
    x[1], a_prev[1] = torch.randn(C, H, W, generator=g), torch.randn(C, H, W, generator=g)
    other = _launch(dev, t, "linear", par, eps=eps.view(-1, LDE), x=x, a_prev=a_prev)
    for k in ("prev", "x0", "eps_out", "A"):
        assert same_bits(base[k][0], other[k][0]) and not same_bits(base[k][1], other[k][1]), k
    assert same_bits(base["sa"][:2], other["sa"][:2]) and not same_bits(base["sa"][2:], other["sa"][2:])


@pytest.mark.parametrize("form", ["linear", "hist"])
def test_restore_map_selects_bits(dev, form):
    from instantir_amd import ops
    shape = SHAPES[0]
    t = _case(shape)
    B, H, W = shape
    g = torch.Generator().manual_seed(21)
    kmap = (torch.rand(B, H * W, generator=g)).to(dev)
    kmap[:, :4] = torch.tensor([0.0, 0.5, float(np.nextafter(np.float32(0.5), np.float32(1))), 1.0], device=dev)
    src, nz0 = torch.randn(B, C, H, W, generator=g).to(dev), torch.randn(B, C, H, W, generator=g).to(dev)
    a, b = 0.62, 0.78
    kcoef = torch.tensor([0.5, a, b, 0.0], device=dev)
    par = _par(dev, ETA, t["r"], BETA)
    free = _launch(dev, t, form, par)
    got = _launch(dev, t, form, par, keep=(kmap, src, nz0, kcoef))
    kept = (kmap <= 0.5).reshape(B, 1, H, W).expand(B, C, H, W)
    assert kept.reshape(B, C, H * W)[0, 0, :4].tolist() == [True, True, False, False]
    keep_val = ops.axpby_f32(src, nz0, torch.tensor([a, b], device=dev), torch.empty_like(src))
    torch.cuda.synchronize()
    assert same_bits(got["prev"][~kept], free["prev"][~kept])          # a free element: the APG launch without a map
    assert same_bits(got["prev"][kept], keep_val[kept])                # a kept element: add_noise
    assert not same_bits(got["prev"][kept], free["prev"][kept])
    for k in ("x0", "A", "sa") + (("hist",) if form == "hist" else ("eps_out",)):
        assert same_bits(got[k], free[k]), k


def test_x0_is_the_kernels_own(dev):
    """x0_out = (x - sb*eps)/sa of the eps the kernel formed (fp32, the statement's op order); the history plane holds it too."""
    shape = SHAPES[1]
    t = _case(shape)
    par = _par(dev, ETA, t["r"], BETA)
    out = _launch(dev, t, "linear", par)
    sb, sa = [torch.tensor(v, dtype=torch.float32) for v in _coef("linear")[1:3]]
    want = (t["x"] - sb * out["eps_out"].cpu()) / sa
    assert same_bits(out["x0"], want)
    h = _launch(dev, t, "hist", par)
    assert same_bits(h["hist"], h["x0"]) and same_bits(h["x0"], out["x0"])


def test_existing_entries_keep_their_bits(dev):
    """iir_sched_step, _hist, _pag and _keep (null APG group) against the fp32 statements of loop_ref.ref_step."""
    from instantir_amd import ops
    B, H, W = SHAPES[0]
    HW = H * W
    g = torch.Generator().manual_seed(33)
    eps16 = torch.randn(3 * B * HW, LDE, generator=g).half()
    x, m, nz = torch.randn(B, C, H, W, generator=g) * 3, torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g)
    e = eps16.float()[:, :C].reshape(3 * B, H, W, C).permute(0, 3, 1, 2)
    u, c, p = e[:B], e[B:2 * B], e[2 * B:]
    s = 2.75
    ps = torch.tensor([s], device=dev)
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)
    e_cfg = u + f32(6.5) * (c - u)
    e_pag = e_cfg + f32(s) * (c - p)
    D = lambda v: v.to(dev)
    for name, form, eg, kw in (("iir_sched_step", "linear", e_cfg, {}), ("iir_sched_step_hist", "hist", e_cfg, dict(hist=True)),
                               ("iir_sched_step_pag", "linear", e_pag, dict(pag_scale=ps)),
                               ("iir_sched_step_keep", "hist", e_pag, dict(pag_scale=ps, hist=True, keep=True))):
        coef = _coef(form)
        want, want_x0 = lr.ref_step(eg, x, coef, m if form == "hist" else None, nz)
        prev, x0 = torch.full((B, C, H, W), 7.0, device=dev), torch.full((B, C, H, W), 7.0, device=dev)
        hist = D(m.clone()) if kw.get("hist") else None
        keep = kept = None
        if kw.get("keep"):
            kmap = torch.rand(B, HW, generator=g)
            src, n0 = torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g)
            keep = (D(kmap), D(src), D(n0), torch.tensor([0.5, 0.62, 0.78, 0.0], device=dev))
            kept = (kmap <= 0.5).reshape(B, 1, H, W).expand(B, C, H, W)
            want = torch.where(kept, f32(0.62) * src + f32(0.78) * n0, want)
        ops.sched_step(D(eps16), B, torch.tensor(coef, device=dev), D(x), prev, noise=D(nz), cfg=True, x0_out=x0,
                       pag_scale=kw.get("pag_scale"), hist=hist, keep=keep)
        torch.cuda.synchronize()
        print(f"{name}: prev / x0 vs the fp32 statements: {lr.ulps(prev.cpu(), want):.2f} / {lr.ulps(x0.cpu(), want_x0):.2f} ulps")
        assert same_bits(prev, want) and same_bits(x0, want_x0), name
        if hist is not None:
            assert same_bits(hist, want_x0), name


def test_ops_refuse_bad_apg_arguments(dev):
    from instantir_amd import ops
    t = _case(SHAPES[0])
    B = SHAPES[0][0]
    x, eps = t["x"].to(dev), t["eps"].to(dev)
    coef = torch.tensor(_coef("linear"), device=dev)
    prev = torch.empty_like(x)
    A, sa, par = torch.zeros_like(x), torch.zeros(2 * B, device=dev), _par(dev, 0.0, 0.0, 0.0)
    with pytest.raises(ValueError, match="eps_factor"):
        ops.sched_step(eps, B, coef, x, prev, eps_factor=torch.ones(B, device=dev), apg=(A, sa, par))
    with pytest.raises(ValueError, match="cfg"):
        ops.sched_step(eps, B, coef, x, prev, cfg=False, apg=(A, sa, par))
    for bad in ((A[:1], sa, par), (A, sa[:1], par), (A, sa, par.cpu()), (A.double(), sa, par), (A.transpose(2, 3), sa, par)):
        with pytest.raises(ValueError, match="apg"):
            ops.sched_step(eps, B, coef, x, prev, apg=bad)
        with pytest.raises(ValueError, match="apg"):
            ops.apg_project(eps, B, coef, x, bad, ops.apg_workspace(B, dev))
    with pytest.raises(ValueError, match="ws"):
        ops.apg_project(eps, B, coef, x, (A, sa, par), torch.empty(96 * B, device=dev))
    with pytest.raises(RuntimeError):
        ops.apg_project(eps, B, coef, x, (A, sa, par), ops.apg_workspace(B, dev)[:-1])       # too small: refused by the entry


# ---- the denoising loop ----------------------------------------------------------------------------------------------------------
BAR = 50.0
G = 7.0
APG = (0.0, 6.0, -0.5)            # eta, norm_threshold, momentum of the loop tests (the clamp is active at this geometry)
LOOP6 = dict(num_inference_steps=6, preview_start=0.25, control_guidance_end=0.75)


def _oracles(env, loop, **kw):
    """(APG'd, plain) of an oracle loop"""
    return loop(env, guidance_scale=G, guide=lr.apg(G, APG), **kw), loop(env, guidance_scale=G, **kw)


def _apg_pipe(env, par=APG, sched=None):
    pipe = lr.pipe(env, sched)
    if par is not None:
        pipe.enable_apg(*par)
    return pipe


_call = functools.partial(lr.call, guidance_scale=G, **LOOP6)


def _check_loop(tag, got, want, plain):
    p_or = lr.psnr(plain, want)
    p, p_plain = lr.psnr(got, want, "apg." + tag.split()[0]), lr.psnr(got, plain)
    print(f"{tag}: latent PSNR vs APG'd oracle {p:.1f} dB, vs plain oracle {p_plain:.1f} dB; the two oracles {p_or:.1f} dB apart")
    assert p_or < 40.0, p_or                                           # on CPU values alone: a no-op implementation cannot pass
    assert torch.isfinite(got).all() and p >= BAR, p
    assert p_plain < p, (p, p_plain)


def test_loop_matches_apg_oracle(env):
    """Six DDIM steps through every phase (Aggregator-only head, previewed middle, creative tail)."""
    want, plain = _oracles(env, lr.denoise, **LOOP6)
    got = _call(_apg_pipe(env), env[4])
    _check_loop("ddim", got, want, plain)


def test_dpmpp_2m_karras_matches_apg_oracle(env):
    want, plain = _oracles(env, lr.sigma_denoise, kind="dpm", n=6, karras=True, **lr.PHASES)
    got = _call(_apg_pipe(env, sched=lr.sigma_sched("dpm", karras=True)), env[4])
    _check_loop("dpmpp_2m karras", got, want, plain)


def test_graphs_on_off_and_repeat_calls_bit_identical(env):
    """A second call on the cached loop equals the first (the average is reset and beta_t is 0 again), with and without graphs,
    in both scheduler forms."""
    inp = env[4]
    for sched in (None, lr.sigma_sched("dpm", karras=True)):
        pipe = _apg_pipe(env, sched=sched)
        a = _call(pipe, inp, num_inference_steps=3)
        b = _call(pipe, inp, num_inference_steps=3)
        pipe.use_graphs = False
        c = _call(pipe, inp, num_inference_steps=3)
        d = _call(pipe, inp, num_inference_steps=3)
        assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, d)


def test_momentum_enters_at_the_second_step(env):
    inp = env[4]

    def run(m):
        seen = []

        def cb(p, i, t, kw):
            seen.append(kw["latents"].float().cpu().clone())
            return {}
        _call(_apg_pipe(env, (APG[0], APG[1], m)), inp, num_inference_steps=2, callback_on_step_end=cb)
        return seen
    a, b = run(-0.5), run(0.0)
    assert len(a) == 2 and len(b) == 2
    assert torch.equal(a[0], b[0]) and not torch.equal(a[1], b[1])


def test_disable_and_toggling_replay_the_right_graphs(env):
    """never enabled == enabled then disabled; off -> on -> off -> on (other parameters) -> on on ONE pipeline: each call equals
    a fresh pipeline with that setting, bit for bit (the parameters travel in the scalar row: the captured loop is re-used)."""
    inp, n3 = env[4], dict(num_inference_steps=3)
    base = _call(_apg_pipe(env, None), inp, **n3)
    p = _apg_pipe(env)
    p.disable_apg()
    assert p.apg is None and torch.equal(_call(p, inp, **n3), base)
    settings = [None, APG, None, (0.5, 3.0, 0.25), APG]
    fresh = {st: (base if st is None else _call(_apg_pipe(env, st), inp, **n3)) for st in set(settings)}
    pipe = _apg_pipe(env, None)
    loops = []
    for st in settings:
        pipe.disable_apg() if st is None else pipe.enable_apg(*st)
        assert torch.equal(_call(pipe, inp, **n3), fresh[st]), st
        loops.append(pipe._loop_cache[1])
    assert loops[3] is loops[4] and loops[0] is not loops[1]
    assert not torch.equal(fresh[None], fresh[APG]) and not torch.equal(fresh[APG], fresh[settings[3]])


def test_composes_with_pag_restore_map_and_images_per_prompt(env):
    from instantir_amd.schedulers import LCMSingleStepScheduler
    inp = env[4]
    one = {k: (v[:1] if k in ("lq", "pe", "pooled", "npe", "npooled", "init_noise") else v) for k, v in inp.items()}
    one["img"] = inp["img"][:, :1]
    rmap = torch.ones(16, 16)
    rmap[:, :8] = 0.0                                                  # left half: never denoised, comes out as the LQ input

    def run():
        p = _apg_pipe(env)
        p.enable_pag("mid")
        outs = []
        for _ in range(2):
            outs.append(p(image=one["lq"], prompt_embeds=one["pe"], pooled_prompt_embeds=one["pooled"],
                          negative_prompt_embeds=one["npe"], negative_pooled_prompt_embeds=one["npooled"],
                          ip_adapter_image_embeds=[one["img"]], output_type="latent",
                          previewer_scheduler=LCMSingleStepScheduler.from_config(p.scheduler.config),
                          init_noise=torch.cat([one["init_noise"]] * 2), guidance_scale=G, pag_scale=3.0, num_images_per_prompt=2,
                          restore_map=rmap, **LOOP6).images.float().cpu())
        return outs
    a, b = run()
    assert a.shape[0] == 2 and torch.isfinite(a).all() and torch.equal(a, b)
    lq2 = one["lq"].repeat(2, 1, 1, 1)
    assert same_bits(a[..., :8], lq2[..., :8]) and not torch.equal(a[..., 8:], lq2[..., 8:])


def test_cli_apg_equals_python_api(tmp_path, dev):
    from PIL import Image
    import instantir_amd.infer as cli
    src, out = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    Image.fromarray(np.random.default_rng(0).integers(0, 255, (96, 96, 3), dtype=np.uint8)).save(src / "a.png")
    args = cli.build_parser().parse_args(["--test_path", str(src), "--out_path", str(out), "--synthetic", "tiny",
                                          "--num_inference_steps", "4", "--width", "128", "--height", "128", "--batch_size", "1",
                                          "--cfg", "5.0", "--apg", "0.25", "6.0", "-0.5"])
    orig = cli.resize_img
    cli.resize_img = lambda im, **kw: orig(im, max_side=128, min_side=128, **kw)
    try:
        torch.manual_seed(7)               # the synthetic VAE encode draws its eps from the global generator
        cli.main(args, dev)
        im, size = cli.resize_img(Image.open(src / "a.png").convert("RGB"), width=128, height=128)
    finally:
        cli.resize_img = orig
    got = np.asarray(Image.open(out / "a.png"))
    torch.manual_seed(7)
    pipe, lcm = cli.build_pipeline(args, dev)
    pipe.enable_apg(0.25, 6.0, -0.5)
    cfg = pipe.cfg
    g = torch.Generator().manual_seed(42)
    kw = dict(prompt_embeds=torch.randn(1, cfg.text_len, cfg.cross_attention_dim, generator=g),
              pooled_prompt_embeds=torch.randn(1, cfg.pooled_dim, generator=g),
              negative_prompt_embeds=torch.randn(1, cfg.text_len, cfg.cross_attention_dim, generator=g),
              negative_pooled_prompt_embeds=torch.randn(1, cfg.pooled_dim, generator=g),
              ip_adapter_image_embeds=[torch.randn(2, 1, cfg.resampler.seq_len, cfg.resampler.embedding_dim, generator=g)])
    rec = pipe(image=[im], num_inference_steps=4, generator=torch.Generator(device=dev).manual_seed(42), guidance_scale=5.0,
               previewer_scheduler=lcm, preview_start=0.0, control_guidance_end=1.0, **kw).images[0]
    want = np.asarray(rec.resize([size[0], size[1]], Image.BILINEAR))
    assert got.shape == want.shape and np.array_equal(got, want)
