"""GPU: every build of `gemm_kernel` / `gemm8_kernel`, by forced dispatch id, element by element against the fp64 reference and
the derived bound of tests/gemm_conv_ref.py (no tolerance: see that module's docstring).

The id lists are the golden maker's (tests/golden/make_gemm_conv_bits.py), checked first against what the library accepts.  Every
output goes into a buffer with 3 spare rows and 8 spare columns pre-filled with a constant, which must come back untouched;
A-side operands are views of wider buffers.  The hash replay of test_kernels_gpu.py pins the bits of one launch per build against
an older library; this file says whether those values are right, at the geometries the replay does not reach."""
import functools

import pytest
import torch

import gemm_conv_ref as R
from golden import make_gemm_conv_bits as maker

pytestmark = pytest.mark.gpu

FILL = maker.FILL
SEEN = {}          # form -> [largest err / bound, largest err / first-order form, elements != want, elements]: printed, not asserted


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from instantir_amd import lib
    lib.load()          # fails loudly if the HIP library is missing
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def cases(group, form):
    return {"gemm": R.gemm_cases, "gemm8": R.gemm8_cases, "conv": R.conv_cases, "act": R.act_cases}[group](form)


@functools.lru_cache(maxsize=None)
def ref_of(group, form, name):
    return R.reference(*cases(group, form)[name])


def on_dev(t, dev):
    """The same view of a device copy of t's whole storage (strides, offset and the bytes between the rows kept)."""
    if not torch.is_tensor(t):
        return t
    base = torch.empty(0, dtype=t.dtype).set_(t.untyped_storage())
    return torch.as_strided(base.to(dev), tuple(t.shape), t.stride(), t.storage_offset())


def out_buf(rows, cols, dtype, dev, spare_cols=8):
    big = torch.full((rows + 3, cols + spare_cols), FILL, dtype=dtype, device=dev)
    return big, big[:rows, :cols]


@functools.lru_cache(maxsize=None)
def sft():
    case = R.sft_case()
    return case, R.reference(*case)


def launch(case, ref, tile, dev, spare_cols=8):
    """Run one case at `tile`; returns [(whole buffer on the CPU, physical rows, want, bound, first-order form), ...]."""
    from instantir_amd import ops
    kind, spec = case
    kw = {k: on_dev(v, dev) for k, v in spec.items() if k not in ("out_t", "out_dtype", "w8", "a8", "x", "a", "w")}
    M, No = ref.want.shape
    odt = spec.get("out_dtype", ref.dtype)
    rows_total = int(ref.rows.max()) + 1
    outs = []
    if spec.get("out_t") is not None:
        tr = spec["out_t"]
        big, o = out_buf(M, tr, odt, dev, spare_cols)
        tbig, ot = out_buf(No - tr, M, odt, dev)
        kw["out_t"] = (ot, tr)
        outs = [(big, ref.rows, ref.want[:, :tr], ref.bound[:, :tr], ref.first_order[:, :tr]),
                (tbig, torch.arange(No - tr), ref.want[:, tr:].T, ref.bound[:, tr:].T, ref.first_order[:, tr:].T)]
    else:
        big, o = out_buf(rows_total, No, odt, dev, spare_cols)
        outs = [(big, ref.rows, ref.want, ref.bound, ref.first_order)]
    if kind == "conv":
        ops.conv2d(on_dev(spec["x"], dev), on_dev(spec["w"], dev), o, tile=tile, **kw)
    elif kind == "gemm":
        ops.gemm(on_dev(spec["a"], dev), on_dev(spec["w"], dev), o, tile=tile, **kw)
    else:
        q, sc = spec["w8"]
        ops.gemm_fp8(on_dev(spec["a8"], dev), ops.Fp8Weight(on_dev(q, dev), on_dev(sc, dev)), o, tile=tile, **kw)
    torch.cuda.synchronize()
    return [(b.cpu(),) + tuple(rest) for b, *rest in outs]


def check(what, form, results):
    """Margins exactly, values by the bound; returns nothing, asserts with the worst offender."""
    for i, (big, rows, want, bound, first) in enumerate(results):
        got = big.double()
        No = want.shape[1]
        written = torch.zeros(got.shape, dtype=torch.bool)
        written[rows[:, None], torch.arange(No)[None, :]] = True
        stray = int((got[~written] != FILL).sum())
        assert stray == 0, f"{what}[{i}]: {stray} elements outside the view were written"
        g = got[rows][:, :No]
        n, worst = R.compare(g, want, bound)
        seen = SEEN.setdefault(form, [0.0, 0.0, 0, 0])
        if n == 0:
            seen[0], seen[1] = max(seen[0], R.room(g, want, bound)), max(seen[1], R.room(g, want, first))
            seen[2], seen[3] = seen[2] + int((g != want).sum()), seen[3] + want.numel()
        assert n == 0, f"{what}[{i}]: {n}/{want.numel()} elements outside the bound, worst {worst}"


def run(group, form, name, tile, dev, spare_cols=8, tag=""):
    check(f"{group}.{form}.{name}{tag}.tile{tile}", form, launch(cases(group, form)[name], ref_of(group, form, name), tile, dev, spare_cols))


# ---- the id lists are the builds the library has ------------------------------------------------------------------------------------
def _accepted(fn):
    """Forced ids 10 .. 99 the library launches (a refusal is IIR_EINVAL from dispatch() / launch(), before anything runs).  The
    wrappers name a launch by the base shape id % 10, so the ids they can hand over end in 0 .. 6.  The try / except belongs to this
    probe alone; the cases below launch bare, so a refused id fails them.  Acceptance can also depend on the shape (the 8-wave
    kernel wants whole 256 x BN tiles and K >= 128): the probe's shape is one every build takes, so it lists builds, not domains."""
    from instantir_amd import lib
    ok = []
    for t in (t for t in range(10, 100) if t % 10 <= 6):
        try:
            fn(t)
            ok.append(t)
        except lib.HipLibraryError as e:
            if "invalid argument" not in str(e):
                raise
    torch.cuda.synchronize()
    return ok


def test_id_lists_are_the_builds_of_the_library(dev):
    """Probe every forced id with whole-tile launches (256 x 1280 x 128; conv 16 x 16, Cin 64 -> Cout 1280): what dispatch() and
    launch() of csrc/gemm_conv.hip accept per element type is exactly the golden maker's lists (fp16: + 90 for paired epilogues, + 91 / 92,
    the 8-wave kernel; all-fp8: + 91)."""
    from instantir_amd import ops
    M, N, K = 256, 1280, 128
    g = torch.Generator().manual_seed(1)
    rnd = lambda *s, dt=torch.float16: (torch.randn(*s, generator=g) / 8).to(dt).to(dev)
    for dt, ids in ((torch.float16, maker.F16_GEMM_IDS), (torch.bfloat16, maker.BF16_IDS)):
        a, w, o, o2 = rnd(M, K, dt=dt), rnd(N, K, dt=dt), torch.empty(M, N, dtype=dt, device=dev), torch.empty(M, N // 2, dtype=dt, device=dev)
        f16 = dt == torch.float16
        assert _accepted(lambda t: ops.gemm(a, w, o, tile=t)) == sorted(ids + ([91, 92] if f16 else [])), dt
        assert _accepted(lambda t: ops.gemm(a, w, o2, epi=ops.EPI_GEGLU, tile=t)) == sorted(ids + ([90, 91, 92] if f16 else [])), dt
        x, wc = rnd(1, 16, 16, 64, dt=dt), rnd(N, 3, 3, 64, dt=dt)
        cids = maker.F16_CONV_IDS if f16 else maker.BF16_IDS
        assert _accepted(lambda t: ops.conv2d(x, wc, o, tile=t)) == sorted(cids), dt
        assert _accepted(lambda t: ops.conv2d(x, wc, o2, res=o2.clone(), epi=ops.EPI_SFT, tile=t)) == sorted(cids + ([90] if f16 else [])), dt
    a, o = rnd(M, K), torch.empty(M, N, dtype=torch.half, device=dev)
    w8 = ops.Fp8Weight(*ops.quantize_fp8_rows(rnd(N, K)))
    assert _accepted(lambda t: ops.gemm(a, w8, o, tile=t)) == sorted(maker.W8_IDS)
    a8, sa = ops.quantize_fp8_tensor(rnd(M, 2 * K))
    w88 = ops.Fp8Weight(*ops.quantize_fp8_rows(rnd(N, 2 * K)))
    assert _accepted(lambda t: ops.gemm_fp8(a8, w88, o, a_scale=sa, tile=t)) == sorted(maker.F8_IDS + [91])


# ---- GEMM, per build ------------------------------------------------------------------------------------------------------------------
GEMM_BUILDS = [("f16", t) for t in [0] + maker.F16_GEMM_IDS] + [("bf16", t) for t in [0] + maker.BF16_IDS] + \
              [("w8", t) for t in [0] + maker.W8_IDS] + [("f8", t) for t in [0] + maker.F8_IDS]


@pytest.mark.parametrize("form,tile", GEMM_BUILDS, ids=[f"{f}-tile{t}" for f, t in GEMM_BUILDS])
def test_gemm_build(dev, form, tile):
    """(a) ragged 300 x 336: bias + row bias + residual + SiLU, out_scale 0.5; (b) whole tiles 512 x 640: bias + residual, the fast
    write-out; (c) the same with ldc % 8 != 0, the non-vector write-out; (d) GEGLU at both shapes; fp16 / bf16 also (e) `out_t` with
    tr_from inside a 128-column tile (C = 160) and on a tile edge (C = 320) and (f) fp32 output.  K = 320."""
    for name in cases("gemm", form):
        run("gemm", form, name, tile, dev)
    run("gemm", form, "b", tile, dev, spare_cols=12, tag="(ldc % 8 = 4)")
    print(f"room {form} after gemm tile {tile}: {SEEN[form]}")


G8_BUILDS = [("f16", 91), ("f16", 92), ("f8", 91)]


@pytest.mark.parametrize("form,tile", G8_BUILDS, ids=[f"{f}-tile{t}" for f, t in G8_BUILDS])
def test_gemm8_build(dev, form, tile):
    """The 8-wave kernel of csrc/gemm8.hip at 256 x 1280 x 320 (the golden maker's shape): bias + residual, and GEGLU."""
    for name in cases("gemm8", form):
        run("gemm8", form, name, tile, dev)
    print(f"room {form} after gemm8 tile {tile}: {SEEN[form]}")


def test_gemm_paired_only_build_90(dev):
    for name in ("d1", "d2"):
        run("gemm", "f16", name, 90, dev)


# ---- conv, per build ------------------------------------------------------------------------------------------------------------------
CONV_BUILDS = [("f16", t) for t in [0] + maker.F16_CONV_IDS] + [("bf16", t) for t in [0] + maker.BF16_IDS]


@pytest.mark.parametrize("form,tile", CONV_BUILDS, ids=[f"{f}-tile{t}" for f, t in CONV_BUILDS])
def test_conv_build(dev, form, tile):
    """Cin 64, non-square maps.  (a) 3 x 3, R = 2, 10 x 14 -> Cout 168: every tile shape straddles the image boundary and is ragged in
    M and N; bias + per-image row bias + residual + SiLU; (b) 16 x 16 -> Cout 640, whole tiles; (c) stride 2 with pad_mode 0, and
    with pad_mode 1 on 11 x 15 and on 10 x 14 (the even map is the one whose last taps read the padding); (d) the folded 2x upsample
    from 5 x 7; (e) 1 x 1 with one and with two K tiles, fewer than a 3-deep ring's prologue; (f) = (a) with remapped output and
    residual rows and a padded image stride."""
    for name in cases("conv", form):
        run("conv", form, name, tile, dev)
    print(f"room {form} after conv tile {tile}: {SEEN[form]}")


@pytest.mark.parametrize("tile", [0, 90])
def test_conv_sft_build(dev, tile):
    """SFT, h * (gamma + 1) + beta, on geometry (a) with Cout 176: the automatic tile and the paired-only 256 x 320 build."""
    check(f"conv.f16.sft.tile{tile}", "f16", launch(*sft(), tile, dev))
    print(f"room f16 after sft tile {tile}: {SEEN['f16']}")


# ---- activations (tile 0) ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["f16", "bf16", "w8", "f8"])
def test_gelu_and_quick_gelu(dev, form):
    """ACT_GELU against exact-erf GELU, ACT_QUICKGELU against x * sigmoid(1.702 x), on GEMM (a) and conv (a)."""
    for name in cases("act", form):
        run("act", form, name, 0, dev)
    print(f"room {form} after the activations: {SEEN[form]}")


# ---- the 2 GiB store switch -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [0, 24, 54, 91])
@pytest.mark.parametrize("ldc", [2 ** 21, 2 ** 21 - 8], ids=["plain-stores", "buffer-stores"])
def test_store_switch_at_2_gib(dev, ldc, tile):
    """finish_geo() of csrc/gemm_conv.hip swaps the 31-bit buffer store of `store16` for plain stores at M * ldc * 2 >= 2 GiB.
    512 x 640 x 64, bias + residual, whole tiles, as a column slice of a (512, ldc) buffer: ldc = 2^21 takes the plain stores,
    2^21 - 8 the buffer store at its largest offsets.  The automatic tile, one 4-wave build, the 128 x 160 loader-wave build and the
    8-wave kernel (K = 128 there: it refuses fewer than two K tiles).  Only the 8 columns beside the view are filled and compared."""
    from instantir_amd import ops
    M, N, _ = R.BIG
    case = R.big_case(128 if tile == 91 else R.BIG[2])
    ref = R.reference(*case)
    s = case.spec
    buf = torch.empty(M, ldc, dtype=torch.half, device=dev)
    assert (M * buf.stride(0) * 2 >= 2 ** 31) == (ldc == 2 ** 21)
    buf[:, N:N + 8] = FILL
    ops.gemm(on_dev(s["a"], dev), on_dev(s["w"], dev), buf[:, :N], bias=on_dev(s["bias"], dev), res=on_dev(s["res"], dev), tile=tile)
    torch.cuda.synchronize()
    got = buf[:, :N + 8].cpu().double()
    del buf
    torch.cuda.empty_cache()
    assert (got[:, N:] == FILL).all(), "the columns beside the view were written"
    n, worst = R.compare(got[:, :N], ref.want, ref.bound)
    assert n == 0, f"tile {tile}, ldc {ldc}: {n}/{ref.want.numel()} elements outside the bound, worst {worst}"
