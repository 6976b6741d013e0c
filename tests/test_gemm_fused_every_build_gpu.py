"""GPU: what every build of `gemm_kernel` / `gemm8_kernel` does beside its matrix product -- the LayerNorm fold (`ln_in`), the
LayerNorm and GroupNorm partials it leaves (`ln_out`, `gn_out`) and the fp8 store (`c_fp8`) -- by forced dispatch id, against the
fp64 references and derived bounds of tests/gemm_fused_ref.py (no tolerance: see that module's docstring).

First the acceptance tables: which build takes which pointer is probed id by id and held against the literal lists of the
reference module.  Outputs and partial buffers are views of wider buffers filled with a constant that must come back untouched;
every partial buffer is pre-filled with NaN and must be finite after the launch.  A statistics launch must store bit for bit what
the same build stores without the pointer; its partials are judged against the fp64 statistics of THOSE stored values; `gn_out`
partials then feed `ops.groupnorm(partials=)`, judged by tests/norm_ref.py.  Every launch prints, and appends to
profiles/gemm_fused_every_build.log: case | build | elements | != want | err / bound of the kernel | of the fp32 stand-in | ms.
One MI355X: 100 tests, 895 launches judged, 3.6 s wall in the file inside the whole suite, 5.3 s alone (7.5 s for pytest, the references on the CPU included)."""
import ctypes
import functools
import os
import time

import numpy as np
import pytest
import torch

import gemm_conv_ref as R
import gemm_fused_ref as FR
import norm_ref as NR
from test_gemm_conv_every_build_gpu import FILL, _accepted, check, on_dev, out_buf

pytestmark = pytest.mark.gpu

LOG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "gemm_fused_every_build.log")
_log_started = []
NAN = float("nan")
IIR_DT = {torch.float16: 0, torch.bfloat16: 1}
FILL8 = 0x55


def log(line):
    """(The figures are printed too; a read-only checkout keeps the test, not the log.)"""
    print(line)
    try:
        with open(LOG, "a" if _log_started else "w") as f:
            if not _log_started:
                f.write(FR.LOG_HEADER + "   (wall ms: launch + sync, not a benchmark)\n")
                _log_started.append(1)
            f.write(line + "\n")
    except OSError:
        pass


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from instantir_amd import lib
    lib.load()          # fails loudly if the HIP library is missing
    t0 = time.perf_counter()
    yield torch.device("cuda:0")
    log(f"# wall time of the file: {time.perf_counter() - t0:.1f} s")


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


# ---- buffers --------------------------------------------------------------------------------------------------------------------------
def stats_buf(shape, dev):
    """(whole flat fp32 buffer, the contiguous view a launch writes): 64 floats of margin on either side hold FILL, the view NaN."""
    n = int(np.prod(shape))
    big = torch.full((n + 128,), FILL, dtype=torch.float32, device=dev)
    big[64:64 + n] = NAN
    return big, big[64:64 + n].view(*shape)


def stats_back(big, shape, what):
    """The view on the CPU; the margins untouched, every element written and finite."""
    n = int(np.prod(shape))
    host = big.cpu()
    assert bool((host[:64] == FILL).all()) and bool((host[64 + n:] == FILL).all()), f"{what}: the partial buffer was written outside its view"
    v = host[64:64 + n].view(*shape)
    bad = int((~torch.isfinite(v)).sum())
    assert bad == 0, f"{what}: {bad}/{v.numel()} partials were not written (still NaN) or are not finite"
    return v


def stats_in(part, dev):
    """Input partials as a view of a wider buffer (the kernel must index [parts][M] inside it)."""
    big = torch.full((part.numel() + 128,), NAN, dtype=torch.float32, device=dev)
    big[64:64 + part.numel()] = part.reshape(-1).to(dev)
    return big[64:64 + part.numel()].view(*part.shape)


def raw_gemm_desc(s, out, tile, ln_out=None):
    """`lib.GemmDesc` of a plain-epilogue launch filled directly: `ops.gemm` refuses `ln_out` with a forced tile."""
    from instantir_amd import lib
    a, w = s["a"], s["w"]
    d = lib.GemmDesc()
    d.A, d.lda, d.W = a.data_ptr(), a.stride(0), w.data_ptr()
    d.C, d.ldc = out.data_ptr(), out.stride(0)
    d.M, d.N, d.K = a.shape[0], w.shape[0], a.shape[1]
    d.bias = s["bias"].data_ptr() if s.get("bias") is not None else None
    if s.get("res") is not None:
        d.res, d.ldr = s["res"].data_ptr(), s["res"].stride(0)
    d.epi, d.act, d.out_scale, d.tile, d.dtype = lib.EPI_PLAIN, lib.ACT_NONE, 1.0, tile, IIR_DT[a.dtype]
    if s.get("wscale") is not None:
        d.wscale = s["wscale"].data_ptr()
    if ln_out is not None:
        d.ln_stats_out = ln_out.data_ptr()
    return d


def raw_gemm(s, out, tile, ln_out=None):
    from instantir_amd import lib
    d = raw_gemm_desc(s, out, tile, ln_out)
    lib.check(lib.load().iir_gemm_f16(ctypes.byref(d), torch.cuda.current_stream().cuda_stream), "iir_gemm_f16")


def operands(spec, dev):
    return {k: on_dev(v, dev) for k, v in spec.items() if torch.is_tensor(v)}


def untouched(big, rows, cols, what):
    host = big.cpu()
    outside = torch.ones(host.shape, dtype=torch.bool)
    outside[:rows, :cols] = False
    fill = FILL8 if host.dtype == torch.uint8 else FILL
    stray = int((host[outside].float() != fill).sum())
    assert stray == 0, f"{what}: {stray} elements outside the view were written"
    return host[:rows, :cols]


# ---- which builds take what ---------------------------------------------------------------------------------------------------------------
def test_acceptance_tables_are_what_the_library_takes(dev):
    """Every forced id, whole-tile launches (256 x 1280 x 128; conv 16 x 16, Cin 64 -> Cout 1280) as in
    test_id_lists_are_the_builds_of_the_library: once with `ln_stats_out`, once with `gn_stats_out` (GEMM and conv), once with
    `c_fp8`.  The accepted sets are the literal lists of tests/gemm_fused_ref.py (derived there from ln_out_fits / gn_out_fits /
    launch_k / gemm8_covers / fill_gemm_geo).  Then iir_gemm_ln_parts / iir_gemm_gn_supported / iir_gemm_fp8_out_supported against
    the tile = 0 launch itself at the shapes this file runs."""
    from instantir_amd import lib, ops
    M, N, K = 256, 1280, 128
    g = torch.Generator().manual_seed(1)
    rnd = lambda *s, dt=torch.float16: (torch.randn(*s, generator=g) / 8).to(dt).to(dev)
    lnp = torch.empty(N // 64, M, 2, dtype=torch.float32, device=dev)
    gnp = torch.empty(M // 64, N, 2, dtype=torch.float32, device=dev)
    for form, dt in (("f16", torch.float16), ("bf16", torch.bfloat16)):
        a, w, o = rnd(M, K, dt=dt), rnd(N, K, dt=dt), torch.empty(M, N, dtype=dt, device=dev)
        assert _accepted(lambda t: raw_gemm(dict(a=a, w=w), o, t, lnp)) == sorted(FR.LN_OUT_IDS[form]), form
        assert _accepted(lambda t: ops.gemm(a, w, o, tile=t, gn_out=gnp)) == sorted(FR.GN_OUT_GEMM_IDS[form]), form
        x, wc = rnd(1, 16, 16, 64, dt=dt), rnd(N, 3, 3, 64, dt=dt)
        assert _accepted(lambda t: ops.conv2d(x, wc, o, tile=t, gn_out=gnp)) == sorted(FR.GN_OUT_CONV_IDS[form]), form
    a, o = rnd(M, K), torch.empty(M, N, dtype=torch.half, device=dev)
    q, sc = ops.quantize_fp8_rows(rnd(N, K))
    assert _accepted(lambda t: raw_gemm(dict(a=a, w=q, wscale=sc), o, t, lnp)) == sorted(FR.LN_OUT_IDS["w8"])
    assert _accepted(lambda t: ops.gemm(a, ops.Fp8Weight(q, sc), o, tile=t, gn_out=gnp)) == sorted(FR.GN_OUT_GEMM_IDS["w8"])
    a8, sa = ops.quantize_fp8_tensor(rnd(M, 2 * K))
    w88 = ops.Fp8Weight(*ops.quantize_fp8_rows(rnd(N, 2 * K)))
    o8 = torch.empty(M, N, dtype=torch.uint8, device=dev)
    assert _accepted(lambda t: ops.gemm_fp8(a8, w88, o8, a_scale=sa, tile=t)) == sorted(FR.C_FP8_IDS)

    def takes(fn):
        try:
            fn()
            return True
        except lib.HipLibraryError as e:
            if "invalid argument" not in str(e):
                raise
            return False
    for Ms, Ns, Ks in ((FR.PM, FR.PN, FR.PK), (256, 320, 320), (M, N, K), (300, 336, 320)):
        a, w, o = rnd(Ms, Ks), rnd(Ns, Ks), torch.empty(Ms, Ns, dtype=torch.half, device=dev)
        d = raw_gemm_desc(dict(a=a, w=w), o, 0)
        rid = lib.load().iir_gemm_resolve_tile(ctypes.byref(d))
        bn = FR.BUILDS[rid].bn
        took = takes(lambda: raw_gemm(dict(a=a, w=w), o, 0, torch.empty(Ns // bn + 1, Ms, 2, dtype=torch.float32, device=dev)))
        assert took == (rid in FR.LN_OUT_IDS["f16"] and Ms % FR.BUILDS[rid].bm == 0 and Ns % bn == 0), (Ms, Ns, Ks, rid)
        # (the consumer holds at most 8 partials per row: more than that the helper reports as 0 although the producer would write them)
        assert ops.ln_parts(Ms, Ns, Ks) == (Ns // bn if took and Ns // bn <= 8 else 0), (Ms, Ns, Ks, rid)
        if Ms % 64 == 0:
            gp = torch.empty(Ms // 64, Ns, 2, dtype=torch.float32, device=dev)
            assert ops.gn_supported(Ms, Ns, Ks) == takes(lambda: ops.gemm(a, w, o, gn_out=gp)), (Ms, Ns, Ks, rid)
        else:
            assert not ops.gn_supported(Ms, Ns, Ks)
    for H, stride in ((16, 1), (32, 2)):
        x, wc = rnd(2, H, H, 64), rnd(FR.PN, 3, 3, 64)
        o, gp = torch.empty(512, FR.PN, dtype=torch.half, device=dev), torch.empty(8, FR.PN, 2, dtype=torch.float32, device=dev)
        assert ops.gn_supported(512, FR.PN, 576, True) == takes(lambda: ops.conv2d(x, wc, o, stride=stride, gn_out=gp))
    for Ms, Ns in (R.G2, R.G1, R.G8):
        a8, sa = ops.quantize_fp8_tensor(rnd(Ms, 640))
        w88 = ops.Fp8Weight(*ops.quantize_fp8_rows(rnd(Ns, 640)))
        o8 = torch.empty(Ms, Ns + 8, dtype=torch.uint8, device=dev)[:, :Ns]
        assert ops.fp8_out_supported(Ms, Ns, 640) == takes(lambda: ops.gemm_fp8(a8, w88, o8, a_scale=sa)), (Ms, Ns)
    torch.cuda.synchronize()


# ---- producers ------------------------------------------------------------------------------------------------------------------------------
def produce(case, tile, dev, stat, spare_cols=8, alias=False):
    """One producer launch with (`stat` = "ln" / "gn") and one without the statistics pointer, into equal buffers.
    -> (stored output on the CPU, partials on the CPU or None, ms of the statistics launch).  Asserts: the two stored buffers are
    bit-equal, nothing beside the views is written, every partial is finite.  alias: the residual IS the output (`res is out`)."""
    from instantir_amd import ops
    kind, spec = case
    s = operands(spec, dev)
    M, N = (spec["a"].shape[0] if kind == "gemm" else 512), spec["w"].shape[0]
    dt = (spec["a"] if kind == "gemm" else spec["x"]).dtype
    outs = []
    for with_stats in (True, False):
        big, o = out_buf(M, N, dt, dev, spare_cols)
        sl = dict(s)
        if alias:
            o.copy_(s["res"])
            sl["res"] = o
        kw = {k: sl[k] for k in ("bias", "res", "rowbias") if k in sl}
        if "rowbias" in sl:
            kw["rows_per_rb"] = spec["rows_per_rb"]
        pbig = shape = None
        if with_stats:
            shape = (N // FR.BUILDS[tile].bn, M, 2) if stat == "ln" else (M // 64, N, 2)
            pbig, pv = stats_buf(shape, dev)
        if kind == "conv":
            fn = lambda: ops.conv2d(sl["x"], sl["w"], o, stride=spec["stride"], tile=tile, gn_out=pv if with_stats else None, **kw)
        elif stat == "ln":
            fn = lambda: raw_gemm(sl, o, tile, pv if with_stats else None)
        else:
            fn = lambda: ops.gemm(sl["a"], sl["w"], o, tile=tile, wscale=sl.get("wscale"), gn_out=pv if with_stats else None, **kw)
        ms = timed(fn)
        outs.append((big, pbig, shape, ms))
    what = f"{kind}.{stat}_out.tile{tile}"
    (big, pbig, shape, ms), (big0, _, _, _) = outs
    stored = untouched(big, M, N, what)
    assert torch.equal(stored.view(torch.int16), untouched(big0, M, N, what).view(torch.int16)), f"{what}: the statistics path changed the stored output"
    return stored, stats_back(pbig, shape, what), ms


@functools.lru_cache(maxsize=None)
def producer(form, op, what):
    return FR.producer_cases(form, op)[what]


LN_OUT_BUILDS = [(f, t) for f in ("f16", "bf16", "w8") for t in FR.LN_OUT_IDS[f]]


@pytest.mark.parametrize("form,tile", LN_OUT_BUILDS, ids=[f"{f}-tile{t}" for f, t in LN_OUT_BUILDS])
def test_ln_out_build(dev, form, tile):
    """512 x 640 x 320, bias (+ residual): `res` with ldc = N + 8 and dense, `res` with the residual aliasing the output (as the
    engine launches ff2 and to_out), residual rows about +-100 spreads, and weight rows [0, 320) zeroed without a residual: the row
    tiles wholly inside are constant, so their M2 must be exactly 0 and their mean exact."""
    bn = FR.BUILDS[tile].bn
    for what, kw in (("res", {}), ("res", dict(spare_cols=0)), ("res", dict(alias=True)), ("rowmean", {}), ("const", {})):
        stored, part, ms = produce(producer(form, "gemm", what), tile, dev, "ln", **kw)
        ref = FR.ln_out_reference(stored.double(), bn)
        n, room, worst = FR.stats_compare(part, ref)
        _, room_s, _ = FR.stats_compare(FR.ln_out_standin(stored.float().numpy(), bn), ref)
        tag = what + "".join(f".{k}" for k in kw)
        differ = int((part[..., 0].double() != ref.mean).sum() + (part[..., 1].double() != ref.m2).sum())
        log(FR.log_line(f"ln_out.{form}.{tag}", tile, part.numel(), differ, room, room_s, ms))
        assert n == 0, f"ln_out {form} {tag} tile {tile}: {n}/{part.numel()} partials outside the bound, {worst}"
        if what == "const":
            t = part[:FR.CONST_COLS // bn]
            assert bool((t[..., 0] == 0.8125).all()) and bool((t[..., 1] == 0).all()), "a constant row tile: mean exact, M2 = 0"


GN_OUT_BUILDS = [(f, "gemm", t) for f in ("f16", "bf16") for t in FR.GN_OUT_GEMM_IDS[f]] + \
                [(f, "conv", t) for f in ("f16", "bf16") for t in FR.GN_OUT_CONV_IDS[f]]


@pytest.mark.parametrize("form,op,tile", GN_OUT_BUILDS, ids=[f"{f}-{o}-tile{t}" for f, o, t in GN_OUT_BUILDS])
def test_gn_out_build(dev, form, op, tile):
    """GEMM 512 x 640 x 320; conv R = 2, 16 x 16, Cin 64 -> Cout 640 and the stride-2 form from 32 x 32.  Channel offsets of about
    100 spreads, one constant channel (exact), a row bias per image.  The partials then feed `ops.groupnorm(partials=)` (32
    groups, SiLU): judged by the `gnp` reference of tests/norm_ref.py on the stored x and the kernel's own partials."""
    from instantir_amd import ops
    rg = FR.gn_layout(FR.BUILDS[tile])[2]
    dt = R.DTYPES[form]
    for o in (("gemm",) if op == "gemm" else ("conv", "conv2")):
        for what in FR.GN_OUT_WHATS:
            stored, part, ms = produce(producer(form, o, what), tile, dev, "gn")
            ref = FR.gn_out_reference(stored.double(), rg)
            n, room, worst = FR.stats_compare(part, ref)
            _, room_s, _ = FR.stats_compare(FR.gn_out_standin(stored.float().numpy(), rg), ref)
            differ = int((part[..., 0].double() != ref.mean).sum() + (part[..., 1].double() != ref.m2).sum())
            log(FR.log_line(f"gn_out.{form}.{o}.{what}", tile, part.numel(), differ, room, room_s, ms))
            assert n == 0, f"gn_out {form} {o} {what} tile {tile}: {n}/{part.numel()} partials outside the bound, {worst}"
            if what == "constch":
                c = part[:, FR.CONST_CH]
                assert bool((c[:, 0].double() == stored[:, FR.CONST_CH].double().reshape(-1, 64)[:, 0]).all()) and bool((c[:, 1] == 0).all()), "a constant channel: mean exact, M2 = 0"
            # the consumer of the chain
            g = R._gen(f"gn.affine.{form}")
            gm, bt = (1.0 + 0.5 * torch.randn(FR.PN, generator=g)).to(dt), (0.5 * torch.randn(FR.PN, generator=g)).to(dt)
            x = stored.to(dev)
            big, y = out_buf(512, FR.PN, dt, dev)
            ws = ops.gn_workspace(dev, 2, 32)
            ms2 = timed(lambda: ops.groupnorm(x, y, 2, 256, gm.to(dev), bt.to(dev), 1e-5, True, 32, ws, partials=part.to(dev)))
            got = untouched(big, 512, FR.PN, "groupnorm from the producer's partials").double().numpy()
            gref = NR.gnp_reference_of(f"{form}.{o}.{what}", (2, 256, FR.PN, 32), form, stored.double().numpy().reshape(2, 256, FR.PN),
                                       gm.double().numpy(), bt.double().numpy(), part.numpy(), 1e-5, True)
            n2, ratio = NR.compare(got, gref)
            log(FR.log_line(f"gn_out.{form}.{o}.{what}->groupnorm", tile, got.size, int((got != gref.want).sum()), ratio, None, ms2))
            assert n2 == 0, f"groupnorm from the partials of {o} {what} tile {tile}: {n2}/{got.size} outside the bound, worst {NR.worst(got, gref)}"


# ---- the consumer ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ln_in_ref(form, name):
    cases = FR.ln_in_g8_cases() if name.startswith("g8") else FR.ln_in_cases(form)
    case = cases[name]
    ref = R.reference(*case)
    return case, ref, R.room(FR.ln_in_standin(case.spec), ref.want, ref.bound) if "out_t" not in case.spec else None


def ln_in_launch(case, ref, tile, dev):
    """-> ([(whole buffer on the CPU, rows, want, bound, first-order form), ...] for `check`, ms)."""
    from instantir_amd import ops
    spec = case.spec
    s = operands(spec, dev)
    part, colsum, eps = spec["ln_in"]
    kw = {k: s[k] for k in ("bias", "res", "wscale") if k in s}
    kw.update(act=spec.get("act", R.ACT_NONE), epi=spec.get("epi", R.EPI_PLAIN), tile=tile, ln_in=(stats_in(part, dev), colsum.to(dev), eps))
    M, No = ref.want.shape
    dt = spec["a"].dtype
    if spec.get("out_t") is not None:
        tr = spec["out_t"]
        big, o = out_buf(M, tr, dt, dev)
        tbig, ot = out_buf(No - tr, M, dt, dev)
        kw["out_t"] = (ot, tr)
        outs = [(big, ref.rows, ref.want[:, :tr], ref.bound[:, :tr], ref.first_order[:, :tr]),
                (tbig, torch.arange(No - tr), ref.want[:, tr:].T, ref.bound[:, tr:].T, ref.first_order[:, tr:].T)]
    else:
        big, o = out_buf(M, No, dt, dev)
        outs = [(big, ref.rows, ref.want, ref.bound, ref.first_order)]
    ms = timed(lambda: ops.gemm(s["a"], s["w"], o, **kw))
    return [(b.cpu(),) + tuple(rest) for b, *rest in outs], ms


def judge(what, form, tile, results, room_s, ms):
    """The figures of one launch, logged BEFORE the assertion of `check` (margins exactly, values by the bound)."""
    worst, differ, elements = 0.0, 0, 0
    for big, rows, want, bound, _ in results:
        g = big.double()[rows][:, :want.shape[1]]
        err = torch.where(torch.isfinite(g), (g - want).abs(), torch.full_like(g, float("inf")))
        worst = max(worst, float((err / bound).max()))
        differ, elements = differ + int((g != want).sum()), elements + want.numel()
    log(FR.log_line(what, tile, elements, differ, worst, room_s, ms))
    check(f"{what}.tile{tile}", form, results)


LN_IN_BUILDS = [(f, t) for f in ("f16", "bf16", "w8") for t in [0] + FR.LN_IN_IDS[f]]


@pytest.mark.parametrize("form,tile", LN_IN_BUILDS, ids=[f"{f}-tile{t}" for f, t in LN_IN_BUILDS])
def test_ln_in_build(dev, form, tile):
    """Synthetic partials, so that every build sees every merge: (a) ragged 300 x 336 (the clamp min(m0 + ln_lt, M - 1) and the
    element-wise write-out) and (b) whole tiles 512 x 640, K = 640; parts 1, 4, 5, 8 (cols 640, 160, 128, 80); bias + residual + SiLU
    and GEGLU; rows with a mean of +-4 and +-100 spreads and one row of zero variance (rstd = eps^-1/2, the output stays finite)."""
    for name in FR.ln_in_cases(form):
        case, ref, room_s = ln_in_ref(form, name)
        results, ms = ln_in_launch(case, ref, tile, dev)
        judge(f"ln_in.{form}.{name}", form, tile, results, room_s, ms)


@pytest.mark.parametrize("tile", FR.LN_IN_G8_IDS)
def test_ln_in_gemm8_build(dev, tile):
    """The 8-wave kernel at 256 x 1280 x 640, its smallest whole-tile shape with this K: the same merges, plain and GEGLU; on the
    256 x 256 build also `out_t` from column 768 (a tile edge), as the fused q|k|v projection launches it."""
    for name, case in FR.ln_in_g8_cases().items():
        if "out_t" in case.spec and tile != 92:
            continue
        case, ref, room_s = ln_in_ref("f16", name)
        results, ms = ln_in_launch(case, ref, tile, dev)
        judge(f"ln_in.f16.{name}", "f16", tile, results, room_s, ms)


@pytest.mark.parametrize("form", ["f16", "bf16"])
def test_chain_producer_into_consumer_at_tile_0(dev, form):
    """The producer's REAL partials into the consumer, both at tile = 0: 256 x 320 x 320 (5 partials of 64 columns) into 256 x 640 x 320
    with the LayerNorm folded in -- by `ops.LnFold` for fp16; it packs fp16 only, so the bf16 fold is written out here."""
    from instantir_amd import ops
    prod, gamma, beta, w, b = FR.chain_case(form)
    s = operands(prod.spec, dev)
    M, C = prod.spec["a"].shape[0], prod.spec["w"].shape[0]
    parts = ops.ln_parts(M, C, C)
    assert parts == 5
    pbig, pv = stats_buf((parts, M, 2), dev)
    hbig, h = out_buf(M, C, R.DTYPES[form], dev)
    ms = timed(lambda: ops.gemm(s["a"], s["w"], h, bias=s["bias"], res=s["res"], ln_out=pv))
    stored = untouched(hbig, M, C, "chain producer")
    part = stats_back(pbig, (parts, M, 2), "chain producer")
    pref = FR.ln_out_reference(stored.double(), C // parts)
    n, room, worst = FR.stats_compare(part, pref)
    log(FR.log_line(f"chain.{form}.ln_out", 0, part.numel(), int((part[..., 0].double() != pref.mean).sum() + (part[..., 1].double() != pref.m2).sum()),
                    room, FR.stats_compare(FR.ln_out_standin(stored.float().numpy(), C // parts), pref)[1], ms))
    assert n == 0, f"chain {form}: {n} partials outside the bound, {worst}"
    if form == "f16":
        fold = ops.LnFold(w.to(dev), gamma.to(dev), beta.to(dev), bias=b.to(dev), eps=FR.LN_EPS)
        fw, fb, colsum = fold.w, fold.bias, fold.colsum
    else:
        fw = (w.float() * gamma.float()[None, :]).to(torch.bfloat16)
        fb, colsum = (w.float() @ beta.float() + b.float()).to(torch.bfloat16).to(dev), fw.float().sum(dim=1).to(dev)
        fw = fw.to(dev)
    wd = fw.cpu().double()          # colsum: an fp32 sum, in any order, of the STORED folded weight
    assert bool(((colsum.cpu().double() - wd.sum(dim=1)).abs() <= FR.g_(C) * wd.abs().sum(dim=1)).all()), "colsum is not the sum of the stored weight"
    case = R.Case("gemm", dict(a=stored, w=fw.cpu(), bias=fb.cpu(), ln_in=(part, colsum.cpu(), FR.LN_EPS)))
    ref = R.reference(*case)
    big, o = out_buf(M, w.shape[0], R.DTYPES[form], dev)
    ms = timed(lambda: ops.gemm(h, fw, o, bias=fb, ln_in=(pv, colsum, FR.LN_EPS)))
    judge(f"chain.{form}.ln_in", form, 0, [(big.cpu(), ref.rows, ref.want, ref.bound, ref.first_order)],
          R.room(FR.ln_in_standin(case.spec), ref.want, ref.bound), ms)


@pytest.mark.parametrize("form", ["f16", "bf16", "w8"])
def test_rsqrt_term_is_measured_at_tile_0(dev, form):
    """The one measured term: with C_RSQRT at 0, the largest (|got - want| - bound) / (|rstd (acc - mean colsum)| L) over the
    elements of the tile = 0 launches that lie outside the bound; printed and logged (none outside: not positive).  C_RSQRT of the
    reference module is twice the largest figure seen on one MI355X; a card or compiler that needs more fails here."""
    excess, outside = 0.0, 0
    for name, case in FR.ln_in_cases(form).items():
        ref0 = R.reference(case.kind, dict(case.spec, c_rsqrt=0.0))
        results, _ = ln_in_launch(case, ref0, 0, dev)
        big, rows, want, bound, _ = results[0]
        g = big.double()[rows][:, :want.shape[1]]
        over = (g - want).abs() - bound
        outside += int((over > 0).sum())
        excess = max(excess, float((over / FR.rsqrt_scale(case.spec).clamp_min(1e-300)).clamp_min(0).max()))
    log(f"# rsqrt term, {form}, tile 0, {len(FR.ln_in_cases(form))} launches with C_RSQRT = 0: {outside} elements outside, largest excess / scale {excess:.3g}")
    assert excess <= FR.C_RSQRT, f"{form}: rsqrtf needs {excess:.3g}, C_RSQRT is {FR.C_RSQRT:.3g}"


# ---- the fp8 store ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", FR.C_FP8_IDS)
def test_c_fp8_build(dev, tile):
    """All-fp8 builds storing E4M3 bytes, plain (bias + residual) and GEGLU at whole tiles (512 x 640 x 640 bytes; the 8-wave kernel
    256 x 1280): the bytes are `to_e4m3` of the fp16 output of the same build and case, nothing is written beside the byte view;
    the ragged 300 x 336 is refused with IIR_EINVAL before anything is launched."""
    from instantir_amd import lib, ops
    cases = R.gemm8_cases("f8") if tile == 91 else {k: v for k, v in R.gemm_cases("f8").items() if k in ("b", "d2")}
    for name, (_, spec) in cases.items():
        q, sc = spec["w8"]
        a8, w8 = on_dev(spec["a8"], dev), ops.Fp8Weight(q.to(dev), sc.to(dev))
        kw = dict(a_scale=spec["a_scale"], bias=spec["bias"].to(dev), epi=spec.get("epi", R.EPI_PLAIN), tile=tile)
        if spec.get("res") is not None:
            kw["res"] = spec["res"].to(dev)
        M, No = spec["a8"].shape[0], q.shape[0] // (2 if spec.get("epi") == R.EPI_GEGLU else 1)
        big16, o16 = out_buf(M, No, torch.float16, dev)
        big8 = torch.full((M + 3, No + 8), FILL8, dtype=torch.uint8, device=dev)
        ops.gemm_fp8(a8, w8, o16, **kw)
        ms = timed(lambda: ops.gemm_fp8(a8, w8, big8[:M, :No], **kw))
        want = R.to_e4m3(untouched(big16, M, No, "fp16 twin").double())
        got = untouched(big8, M, No, f"c_fp8 {name} tile {tile}").view(torch.float8_e4m3fn).float().double()
        differ = int((got != want).sum())
        log(FR.log_line(f"c_fp8.{name}", tile, want.numel(), differ, None, None, ms))
        assert differ == 0, f"c_fp8 {name} tile {tile}: {differ}/{want.numel()} bytes are not to_e4m3 of the fp16 output"
    _, spec = R.gemm_cases("f8")["a"]
    q, sc = spec["w8"]
    o8 = torch.full((300, 336 + 8), FILL8, dtype=torch.uint8, device=dev)
    with pytest.raises(lib.HipLibraryError, match="invalid argument"):
        ops.gemm_fp8(on_dev(spec["a8"], dev), ops.Fp8Weight(q.to(dev), sc.to(dev)), o8[:, :336], a_scale=spec["a_scale"], tile=tile)
    torch.cuda.synchronize()
    assert bool((o8 == FILL8).all())
