"""GPU: the to_q + cross-attention epilogue (`ops.gemm(..., epi=EPI_XATTN, xattn=(segs, Tq))`, the 64 x 128 tile, dispatch id 93)
at every case of tests/xattn_ref.py, element by element against that module's fp64 reference and derived interval (no
tolerance: see its docstring).

The operands are that module's: every one a view of a wider buffer (lda > K, K a column slice with NaN beside it and NaN in the
rows between Tkv and the batch stride, V^T with NaN around every window and +-1000 on [Tkv, roundup8(Tkv)), strides larger than
needed), O a view inside a sentinel-filled buffer with spare rows and columns.  Every case asserts, over the whole O storage:
  1. the output is finite, 0 elements lie outside [lo, hi], everything outside the view keeps its bits;
  2. no input storage has a changed bit;
  3. a second launch on fresh buffers agrees in every bit;
  4. what follows from each workgroup reading only its own tile's operands, bit for bit: the rows of image b equal the same launch
     for image b alone; columns [128 t, 128 t + 128) equal an N = 128 launch on that slice of W, bias, colsum, K and V^T; flipping
     the V^T pads to the opposite sign, or overwriting the K rows past Tkv with finite values, changes nothing; neither does a
     `prefetch` range.
Each case prints, and appends to profiles/xattn_every_case.log: the kernel's worst err / bound, the share of elements != want, the
fp32 stand-in's worst err / bound for the same case (computed here on the CPU); the file's wall time closes the log.
tests/test_xattn_ref_cpu.py shows that the stand-in stays inside the interval at these cases and that its mutants do not."""
import os
import time

import pytest
import torch

import xattn_ref as X

pytestmark = pytest.mark.gpu

LOG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "xattn_every_case.log")
_log_started = []
_totals = dict(cases=0, elements=0, differ=0, kernel=0.0, standin=0.0, launches=0)


def log(line):
    """(The figures are printed too; a read-only checkout keeps the test, not the log.)"""
    try:
        with open(LOG, "a" if _log_started else "w") as f:
            if not _log_started:
                f.write(X.LOG_HEADER + "\n")
                _log_started.append(1)
            f.write(line + "\n")
    except OSError:
        pass


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    t0 = time.perf_counter()          # the file's wall time: from its first case's setup to its last case (references and copies included)
    from instantir_amd import lib
    lib.load()          # fails loudly if the HIP library is missing
    yield torch.device("cuda:0")
    t = _totals
    if t["cases"]:
        line = (f"# total: {t['cases']} cases, {t['launches']} launches, {t['elements']} elements, != want {100.0 * t['differ'] / t['elements']:.2f} %, "
                f"kernel worst err/bound {t['kernel']:.4f}, stand-in worst err/bound {t['standin']:.4f}, file wall time {time.perf_counter() - t0:.1f} s")
        print(line)
        log(line)


def storage_of(t):
    return torch.empty(0, dtype=t.dtype).set_(t.untyped_storage())


def on_dev(t, dev, keep=None):
    """The same view of a device copy of t's whole storage (strides, offset and everything around the view kept); `keep`
    collects (host storage, device storage) pairs for the unchanged-input check."""
    base = storage_of(t)
    dbase = base.to(dev)
    if keep is not None:
        keep.append((base, dbase))
    return torch.as_strided(dbase, tuple(t.shape), t.stride(), t.storage_offset())


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


class Launch:
    """Device copies of one case's operands (fresh buffers per instance) and the launches made of them."""

    def __init__(self, cs, host, dev):
        self.cs, self.dev, self.keep = cs, dev, []
        s = host.spec
        up = lambda t: on_dev(t, dev, self.keep)
        self.a, self.w = up(s["a"]), up(s["w"])
        self.bias = up(s["bias"]) if s.get("bias") is not None else None
        self.ln_in = None
        if s.get("ln_in") is not None:
            part, colsum, eps = s["ln_in"]
            self.ln_in = (up(part), up(colsum), eps)
        self.kv = [(up(k), rows, up(vt), vbs, tkv) for k, rows, vt, vbs, tkv in host.kv]

    def out_buffer(self, M, C):
        big = torch.full((M + X.SPARE_ROWS, C + 2 * X.BORDER), X.SENTINEL, dtype=torch.half, device=self.dev)
        return big, big[:M, X.BORDER:X.BORDER + C]

    def run(self, rows=None, cols=None, prefetch=None):
        """One launch: the whole case, or the query rows `rows` = (image b alone), or the output columns `cols` = (t: 128 t ..).
        -> (whole O buffer on the CPU, wall ms)."""
        from instantir_amd import ops
        cs = self.cs
        a, w, bias, ln_in, kv, R = self.a, self.w, self.bias, self.ln_in, self.kv, cs.R
        C = cs.heads * 64
        if rows is not None:
            b = rows
            a = a[b * cs.Tq:(b + 1) * cs.Tq]
            if ln_in is not None:
                ln_in = (ln_in[0][:, b * cs.Tq:(b + 1) * cs.Tq].contiguous(), ln_in[1], ln_in[2])
            kv = [(k[b * kr:(b + 1) * kr], kr, vt[:, b * vbs:], vbs, tkv) for k, kr, vt, vbs, tkv in kv]
            R = 1
        if cols is not None:
            c0 = 128 * cols
            w = w[c0:c0 + 128]
            bias = bias[c0:c0 + 128] if bias is not None else None
            if ln_in is not None:
                ln_in = (ln_in[0], ln_in[1][c0:c0 + 128], ln_in[2])
            kv = [(k[:, c0:c0 + 128], kr, vt[c0:c0 + 128], vbs, tkv) for k, kr, vt, vbs, tkv in kv]
            C = 128
        big, o = self.out_buffer(R * cs.Tq, C)
        kw = {}
        if ln_in is not None:
            kw["ln_in"] = ln_in
        if cs.out_scale != 1.0:
            kw["out_scale"] = cs.out_scale
        if prefetch is not None:
            kw["prefetch"] = (prefetch.data_ptr(), prefetch.numel() * prefetch.element_size())
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ops.gemm(a, w, o, bias=bias, epi=ops.EPI_XATTN, xattn=(kv, cs.Tq), **kw)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        _totals["launches"] += 1
        return big.cpu(), ms

    def inputs_unchanged(self):
        return all(torch.equal(bits(h), bits(d.cpu())) for h, d in self.keep)


def split(buf, M, C):
    """(the view's values, True if everything outside the view still holds the sentinel's bits)."""
    outside = torch.ones(buf.shape, dtype=torch.bool)
    outside[:M, X.BORDER:X.BORDER + C] = False
    fill = bits(torch.tensor([X.SENTINEL], dtype=torch.half))[0]
    return buf[:M, X.BORDER:X.BORDER + C], bool((bits(buf)[outside] == fill).all())


@pytest.mark.parametrize("name", list(X.CASES))
def test_xattn_case(dev, name):
    cs = X.CASES[name]
    host = X.operands(cs)
    ref = X.reference(cs, host)
    M, C = cs.R * cs.Tq, cs.heads * 64
    first = Launch(cs, host, dev)
    buf, ms = first.run()
    got, clean = split(buf, M, C)
    # 1. finite, inside the interval, nothing outside the view written
    assert torch.isfinite(got).all(), f"{name}: non-finite output"
    assert clean, f"{name}: something outside the O view was written"
    n, ratio = X.outside(got, ref)
    s_ratio = X.outside(X.standin(cs, host), ref)[1]
    differ = int((got.double() != ref.want).sum())
    line = (f"{name} | {cs.R} x {cs.Tq} x {cs.heads}, {cs.K}, {cs.tk} | {got.numel()} | {100.0 * differ / got.numel():.2f} % | {ratio:.4f} | "
            f"{s_ratio:.4f} | {ms:.2f}")
    print(line)
    log(line)
    t = _totals
    t["cases"] += 1; t["elements"] += got.numel(); t["differ"] += differ
    t["kernel"], t["standin"] = max(t["kernel"], ratio), max(t["standin"], s_ratio)
    assert n == 0, f"{name}: {n}/{got.numel()} elements outside [lo, hi], worst {X.worst(got, ref, cs)}"
    # 2. no input storage has a changed bit
    assert first.inputs_unchanged(), f"{name}: an input buffer was written"
    # 3. a second launch on fresh buffers agrees in every bit
    second = Launch(cs, host, dev)
    buf2, _ = second.run()
    assert torch.equal(bits(buf2), bits(buf)), f"{name}: two launches differ"
    # 4. bit contracts: each workgroup reads its own tile's operands only
    for b in range(cs.R):
        bi, _ = second.run(rows=b)
        gi, clean = split(bi, cs.Tq, C)
        assert clean and torch.equal(bits(gi), bits(got[b * cs.Tq:(b + 1) * cs.Tq])), f"{name}: image {b} alone differs"
    for tcol in range(cs.heads // 2):
        bh, _ = second.run(cols=tcol)
        gh, clean = split(bh, M, 128)
        assert clean and torch.equal(bits(gh), bits(got[:, 128 * tcol:128 * tcol + 128])), f"{name}: head tile {tcol} alone differs"
    pads = Launch(cs, host, dev)
    for k, kr, vt, vbs, tkv in pads.kv:
        tpad = X.roundup8(tkv)
        for b in range(cs.R):
            k[b * kr + tkv:(b + 1) * kr] = 3.0 + b                       # the K rows past Tkv: finite, other values
            if tpad > tkv:
                vt[:, b * vbs + tkv:b * vbs + tpad] = X.pad_values(C, tpad - tkv, b, sign=-1.0).to(dev)
    bp, _ = pads.run()
    assert torch.equal(bits(bp), bits(buf)), f"{name}: the V^T pads or the K rows past Tkv reach the output"
    pf = torch.zeros(64 << 10, dtype=torch.uint8, device=dev)
    bf, _ = second.run(prefetch=pf)
    assert torch.equal(bits(bf), bits(buf)), f"{name}: a prefetch range changes the output"
    assert second.inputs_unchanged() and not bool(pf.any())
