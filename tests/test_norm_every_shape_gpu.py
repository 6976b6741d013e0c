"""GPU: every kernel of csrc/norm.hip through `ops` (GroupNorm in the three-launch and the `partials=` form, LayerNorm plain / adaLN /
transposed / fp8 out, `adaln_batch`, both row softmaxes), element by element against the fp64 reference and the derived bound of
tests/norm_ref.py (no tolerance: see that module's docstring), at the shapes that reach every branch of the kernels.

Inputs are views of wider buffers (ldx > C, ldy > C, ldx != ldy) with NaN in the spare columns and in a row before and after;
outputs sit in buffers whose spare rows and columns hold a constant that must come back untouched; the GroupNorm workspace is
filled with NaN before every launch.  Every case asserts 0 elements outside the bound and appends a line to
profiles/norm_every_shape.log.  tests/test_norm_ref_cpu.py shows that the fp32 stand-ins stay inside the bound at these cases,
that the mutants do not, and what the case table reaches."""
import os
import time

import numpy as np
import pytest
import torch

import norm_ref as R

pytestmark = pytest.mark.gpu

LOG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "norm_every_shape.log")
_log_started = []
NAN = float("nan")


def log(line):
    """(The figures are printed too; a read-only checkout keeps the test, not the log.)"""
    try:
        with open(LOG, "a" if _log_started else "w") as f:
            if not _log_started:
                f.write("# case | elements | worst err/bound | share of elements != want | largest fp32 slack / output ulp | median of the same | "
                        "wall ms (launch + sync, not a benchmark)\n")
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


def wide_in(t, dev, geom, fill=NAN):
    """(whole buffer, view holding t) on the device: `fill` in every spare row and column."""
    nb, ld, r0, c0 = geom
    buf = torch.full((nb, ld), fill, dtype=t.dtype)
    buf[r0:r0 + t.shape[0], c0:c0 + t.shape[1]] = t
    buf = buf.to(dev)
    return buf, buf[r0:r0 + t.shape[0], c0:c0 + t.shape[1]]


def wide_out(shape, dtype, dev, geom):
    nb, ld, r0, c0 = geom
    fill = R.SENTINEL8 if dtype == torch.uint8 else R.SENTINEL
    buf = torch.full((nb, ld), fill, dtype=dtype, device=dev)
    return buf, buf[r0:r0 + shape[0], c0:c0 + shape[1]]


def as64(t):
    t = t.cpu()
    if t.dtype == torch.uint8:
        t = t.view(torch.float8_e4m3fn)
    return t.float().double().numpy()


def split(buf, shape, geom, mask=None):
    """(the view's values as float64, True if everything the launch should not write still holds the fill)."""
    nb, ld, r0, c0 = geom
    host = as64(buf)
    fill = float(as64(torch.tensor([R.SENTINEL8], dtype=torch.uint8))[0]) if buf.dtype == torch.uint8 else R.SENTINEL
    keep = np.ones(host.shape, bool)
    keep[r0:r0 + shape[0], c0:c0 + shape[1]] = False if mask is None else ~mask
    return host[r0:r0 + shape[0], c0:c0 + shape[1]], bool((host[keep] == fill).all())


def judge(cs, got, ref, ms, mask=None, name=None):
    n, _ = R.compare(got, ref, mask)
    ratio, neq, su = R.figures(got, ref, cs, mask)
    med = float(np.median(ref.slack / R.ulp_of(ref.want, cs)))
    line = f"{name or cs.name} | {got.size} | {ratio:.4f} | {neq:.4f} | {su:.3g} | {med:.3g} | {ms:.2f}"
    print(line)
    log(line)
    assert n == 0, f"{name or cs.name}: {n}/{got.size} elements outside the bound, worst {R.worst(got, ref)}"


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


# ---- GroupNorm ----------------------------------------------------------------------------------------------------------------------
def gn_launch(cs, dev, direct_ldp=None):
    from instantir_amd import lib, ops
    Rr, HW, C, G = cs.shape
    o = cs.opt
    xt, _, gm, bt = R.gn_input(cs.shape, cs.dtype, o["mode"])
    xbuf, x = wide_in(xt, dev, R.x_geometry(cs))
    obuf, out = wide_out(x.shape, xt.dtype, dev, R.out_geometry(cs))
    ws = ops.gn_workspace(dev, Rr, G)
    ws.fill_(NAN)
    gm, bt = gm.to(dev), bt.to(dev)
    part = None
    if cs.kind == "gnp":
        p = torch.from_numpy(R.gn_partials(cs.shape, cs.dtype, o["mode"]))
        if direct_ldp is None:
            part = p.to(dev)
        else:                       # the partials as a column slice of a wider fp32 (mean, M2) matrix
            pbuf = torch.full((p.shape[0], direct_ldp, 2), NAN, dtype=torch.float32)
            pbuf[:, 4:4 + C] = p
            pbuf = pbuf.to(dev)
            part = pbuf[:, 4:4 + C]
    if direct_ldp is None:
        ms = timed(lambda: ops.groupnorm(x, out, Rr, HW, gm, bt, o["eps"], o["silu"], G, ws, partials=part))
    else:
        ms = timed(lambda: lib.check(lib.load().iir_groupnorm_from_partials(
            part.data_ptr(), direct_ldp, x.data_ptr(), x.stride(0), out.data_ptr(), out.stride(0), Rr, HW, C, G, gm.data_ptr(), bt.data_ptr(),
            o["eps"], int(o["silu"]), ws.data_ptr(), ws.numel() * 4, 0 if cs.dtype == "f16" else 1, torch.cuda.current_stream().cuda_stream),
            "iir_groupnorm_from_partials"))
    got, clean = split(obuf, x.shape, R.out_geometry(cs))
    assert bool(torch.isnan(xbuf).sum() == xbuf.numel() - x.numel()), "the input buffer changed"
    return got, clean, ms


@pytest.mark.parametrize("name", [n for n, c in R.CASES.items() if c.kind in ("gn", "gnp")])
def test_groupnorm(dev, name):
    cs = R.CASES[name]
    got, clean, ms = gn_launch(cs, dev)
    assert clean, f"{name}: something outside the output view was written"
    judge(cs, got, R.reference(cs), ms)


def test_groupnorm_from_partials_with_a_wider_partial_matrix(dev):
    """`iir_groupnorm_from_partials` with ldp > C (`ops.groupnorm` always passes ldp = C): the same bits as the dense launch."""
    cs = R.CASES["gnp.2x1024x320g32.f16.silu.e5"]
    got, clean, ms = gn_launch(cs, dev, direct_ldp=cs.shape[2] + 8)
    assert clean
    judge(cs, got, R.reference(cs), ms, name=cs.name + ".ldp328")
    assert np.array_equal(got, gn_launch(cs, dev)[0])


# ---- LayerNorm ----------------------------------------------------------------------------------------------------------------------
def ln_launch(cs, dev, via=None):
    """One `ops.layernorm` launch of `cs`; `via(x, out, shift, scale)` replaces the launch (the batched form)."""
    from instantir_amd import ops
    o = cs.opt
    xt, _, gm, bt, sh, sc = R.ln_input(cs.shape)
    xbuf, x = wide_in(xt, dev, R.x_geometry(cs))
    odt = torch.uint8 if o.get("fp8") else torch.half
    obuf, out = wide_out(R.out_shape(cs), odt, dev, R.out_geometry(cs))
    kw = dict(eps=o["eps"])
    if "g" in o["affine"]:
        kw["gamma"] = gm[0].to(dev)
    if "b" in o["affine"]:
        kw["beta"] = bt[0].to(dev)
    if o.get("ada"):
        mod = torch.full((sh[0].shape[0] + 2, 2 * cs.shape[1] + 24), NAN, dtype=torch.half)          # [shift | scale] column slices
        mod[1:-1, 8:8 + cs.shape[1]] = sh[0]
        mod[1:-1, 16 + cs.shape[1]:16 + 2 * cs.shape[1]] = sc[0]
        mod = mod.to(dev)
        kw.update(shift=mod[1:-1, 8:8 + cs.shape[1]], scale=mod[1:-1, 16 + cs.shape[1]:16 + 2 * cs.shape[1]], rows_per_mod=o["rpm"])
    if o.get("tr"):
        kw.update(transposed=True, tr_rows=o["tr_rows"], tr_bstride=o["tr_bstride"])
    if via is None:
        ms = timed(lambda: ops.layernorm(x, out, **kw))
    else:
        ms = timed(lambda: via(x, out, kw["shift"], kw["scale"]))
    mask = R.written_mask(cs)
    got, clean = split(obuf, R.out_shape(cs), R.out_geometry(cs), mask)
    assert bool(torch.isnan(xbuf).sum() == xbuf.numel() - x.numel()), "the input buffer changed"
    return got, clean, ms, mask


@pytest.mark.parametrize("name", [n for n, c in R.CASES.items() if c.kind == "ln"])
def test_layernorm(dev, name):
    cs = R.CASES[name]
    got, clean, ms, mask = ln_launch(cs, dev)
    assert clean, f"{name}: something the launch should not write was written"
    ref = R.reference(cs)
    judge(cs, got, ref, ms, mask)
    if cs.opt.get("fp8"):          # the fp8 store rounds the fp16 value of the same launch
        g16 = ln_launch(cs._replace(opt={k: v for k, v in cs.opt.items() if k != "fp8"}), dev)[0]
        assert np.array_equal(got, R.e4m3(g16)), f"{name}: the fp8 bytes are not E4M3 of the same launch's fp16 output"


def test_adaln_batch(dev):
    """Jobs of C = 8, 320 and 2560 in both orientations, 37 rows (% 4 != 0), one launch: each job bit-equal to its single launch
    and inside the bound."""
    from instantir_amd import ops
    jobs, keep = [], []
    for C, tr in R.ADALN_JOBS:
        cs = R.adaln_case(C, tr)
        ln_launch(cs, dev, via=lambda x, out, sh, sc, tr=tr: jobs.append((x, out, sh, sc, tr)))
    # one modulation matrix for all jobs: the batched launch has a single ldmod
    width = sum(2 * C + 16 for C, _ in R.ADALN_JOBS)
    mod = torch.full((18, width), NAN, dtype=torch.half, device=dev)
    off, table_jobs = 0, []
    for (x, out, sh, sc, tr), (C, _) in zip(jobs, R.ADALN_JOBS):
        mod[1:-1, off:off + C] = sh
        mod[1:-1, off + C + 8:off + 2 * C + 8] = sc
        table_jobs.append((x, out, mod[1:-1, off:off + C], mod[1:-1, off + C + 8:off + 2 * C + 8], tr))
        off += 2 * C + 16
    keep.append(mod)
    table = ops.adaln_job_table(table_jobs, dev)
    ms = timed(lambda: ops.adaln_batch(table, len(table_jobs), 37, 2560, mod.stride(0), 16, 16, 24))
    for (x, out, *_), (C, tr) in zip(table_jobs, R.ADALN_JOBS):
        cs = R.adaln_case(C, tr)
        mask = R.written_mask(cs)
        got = as64(out)
        assert (got[~mask] == R.SENTINEL).all()
        judge(cs, got, R.reference(cs), ms, mask)
        single, clean, _, _ = ln_launch(cs, dev)
        assert clean and np.array_equal(got[mask], single[mask]), f"{cs.name}: the batched launch differs from the single one"


# ---- softmax ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n, c in R.CASES.items() if c.kind == "sm16"])
def test_softmax_rows(dev, name):
    from instantir_amd import ops
    cs = R.CASES[name]
    xt = R.sm_input(cs.kind, cs.shape)[0]
    geom = (cs.shape[0] + 2, cs.shape[1] + 24, 1, 8)
    buf, x = wide_in(xt, dev, geom)
    ms = timed(lambda: ops.softmax_rows(x))
    assert bool(torch.isnan(buf).sum() == buf.numel() - x.numel()), f"{name}: something outside the view was written"
    judge(cs, as64(x), R.reference(cs), ms)


@pytest.mark.parametrize("name", [n for n, c in R.CASES.items() if c.kind == "sm32"])
def test_softmax_rows_f32(dev, name):
    from instantir_amd import ops
    cs = R.CASES[name]
    st = R.sm_input(cs.kind, cs.shape)[0]
    sbuf, s = wide_in(st, dev, (cs.shape[0] + 2, cs.shape[1] + 24, 1, 8))
    geom = (cs.shape[0] + 3, cs.shape[1] + 40, 1, 16)
    pbuf, p = wide_out(cs.shape, R.tdtype(cs.dtype), dev, geom)
    ms = timed(lambda: ops.softmax_rows_f32(s, p))
    got, clean = split(pbuf, cs.shape, geom)
    assert clean, f"{name}: something outside the output view was written"
    assert bool(torch.isnan(sbuf).sum() == sbuf.numel() - torch.isfinite(s).sum() - torch.isinf(s).sum())
    judge(cs, got, R.reference(cs), ms)


# ---- refusals that come after the device test ---------------------------------------------------------------------------------------
def test_wrappers_refuse_what_only_a_device_tensor_can_carry(dev):
    from instantir_amd import lib, ops
    z = lambda *s, dt=torch.half: torch.zeros(*s, dtype=dt, device=dev)
    flat = z(4096)
    over = torch.as_strided(flat, (4, 64), (56, 1))                  # rows that overlap: a row stride below the width
    with pytest.raises(lib.HipLibraryError, match="invalid argument"):
        ops.softmax_rows(over)
    with pytest.raises(lib.HipLibraryError, match="invalid argument"):
        ops.layernorm(over, z(4, 64))
    with pytest.raises(lib.HipLibraryError, match="invalid argument"):
        ops.layernorm(z(4, 64), over)
    with pytest.raises(lib.HipLibraryError, match="invalid argument"):
        ops.groupnorm(over, z(4, 64), 1, 4, z(64), z(64), 1e-5, False)
    with pytest.raises(lib.HipLibraryError, match="invalid argument"):
        ops.groupnorm(z(4, 64), over, 1, 4, z(64), z(64), 1e-5, False)
    with pytest.raises(lib.HipLibraryError, match="invalid argument"):
        ops.softmax_rows_f32(torch.as_strided(z(4096, dt=torch.float32), (4, 64), (60, 1)), z(4, 64))
    with pytest.raises(ValueError):
        ops.groupnorm(z(4, 64), z(4, 64), 1, 4, z(64, dt=torch.bfloat16), z(64), 1e-5, False)
