"""GPU: every build of `attn_kernel2` (head dim 64: every tile staged at entry, the ring for 2 and for 3 waves per SIMD, the identity
form of each) and both builds of `attn_hd_kernel` (80, 104), through `ops.attention`, element by element against the fp64
reference and the derived bound of tests/attention_ref.py (no tolerance: see that module's docstring).

The operands are that module's: Q / K column slices with NaN beside them, NaN in the K rows between Tkv and the batch stride, V^T
with NaN around its window and +-1000 on [Tkv, roundup8(Tkv)), O a view inside a sentinel-filled buffer.  Every case asserts: the
output is finite, nothing outside the view is written, 0 elements outside the bound; identity rows bit-equal to V and the
attending rows bit-equal to the same launch without the identity rows; an fp8 output bit-equal to E4M3 of the same launch's fp16
output.  Each case appends a line to profiles/attention_every_build.log: the kernel's worst err / bound, the used fraction of the
bound, and the fp32 stand-in's worst err / bound for the same case (computed here on the CPU).  tests/test_attention_ref_cpu.py
shows that the stand-ins stay inside the bound at these cases, that the mutants do not, and what the case list reaches."""
import os
import time

import pytest
import torch

import attention_ref as R

pytestmark = pytest.mark.gpu

LOG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "attention_every_build.log")
_log_started = []


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from instantir_amd import lib
    lib.load()          # fails loudly if the HIP library is missing
    return torch.device("cuda:0")


def log(line):
    """(The figures are printed too; a read-only checkout keeps the test, not the log.)"""
    try:
        with open(LOG, "a" if _log_started else "w") as f:
            if not _log_started:
                f.write("# case | build | attending workgroups | elements | != want | kernel worst err/bound | room (used fraction of the bound) | "
                        "stand-in worst err/bound | kernel wall ms (launch + sync, not a benchmark)\n")
                _log_started.append(1)
            f.write(line + "\n")
    except OSError:
        pass


def on_dev(t, dev):
    """The same view of a device copy of t's whole storage (strides, offset and everything around the view kept)."""
    base = torch.empty(0, dtype=t.dtype).set_(t.untyped_storage())
    return torch.as_strided(base.to(dev), tuple(t.shape), t.stride(), t.storage_offset())


def out_buffer(cs, dev, fp8):
    """(whole buffer, view): 3 spare rows below and BORDER columns on either side, pre-filled."""
    rows, C = cs.B * cs.Tq, cs.heads * cs.D
    if fp8:
        big = torch.full((rows + 3, C + 2 * R.BORDER), R.SENTINEL8, dtype=torch.uint8, device=dev)
    else:
        big = torch.full((rows + 3, C + 2 * R.BORDER), R.SENTINEL, dtype=torch.half, device=dev)
    return big, big[:rows, R.BORDER:R.BORDER + C]


def launch(cs, dev, operands, fp8=None, batch=None, ident_from=None):
    """One launch of `cs` on device copies of `operands`; returns (whole O buffer on the CPU as float64, wall ms)."""
    from instantir_amd import ops
    fp8 = cs.o_fp8 if fp8 is None else fp8
    q, kv = operands
    big, o = out_buffer(cs, dev, fp8)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ops.attention(q, o, kv, cs.B if batch is None else batch, cs.heads, cs.Tq, scale=cs.scale, causal=cs.causal, q_prescaled=cs.qpre,
                  head_dim=cs.D, ident_from=cs.ident_from if ident_from is None else ident_from)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    host = big.cpu()
    return (host.view(torch.float8_e4m3fn).float().double() if fp8 else host.double()), ms


def split(cs, buf, fp8):
    """(the view's values, True if everything outside the view still holds the fill)."""
    rows, C = cs.B * cs.Tq, cs.heads * cs.D
    fill = float(torch.tensor([R.SENTINEL8], dtype=torch.uint8).view(torch.float8_e4m3fn).float()) if fp8 else R.SENTINEL
    outside = torch.ones(buf.shape, dtype=torch.bool)
    outside[:rows, R.BORDER:R.BORDER + C] = False
    return buf[:rows, R.BORDER:R.BORDER + C], bool((buf[outside] == fill).all())


@pytest.mark.parametrize("name", list(R.CASES))
def test_attention_build(dev, name):
    cs = R.CASES[name]
    host = R.operands(cs)
    operands = (on_dev(host.q, dev), [(on_dev(k, dev), rows, on_dev(vt, dev), vbs, tkv) for k, rows, vt, vbs, tkv in host.kv])
    ref = R.reference(cs, host)
    buf, ms = launch(cs, dev, operands)
    got, clean = split(cs, buf, cs.o_fp8)
    assert torch.isfinite(got).all(), f"{name}: non-finite output"
    assert clean, f"{name}: something outside the O view was written"
    n, ratio = R.compare(got, ref.want, ref.bound)
    s_ratio = R.compare(R.standin(cs, host), ref.want, ref.bound)[1]
    line = (f"{name} | {R.build_of(cs)} | {R.n_attending(cs)} | {got.numel()} | {int((got != ref.want).sum())} | {ratio:.4f} | "
            f"{R.room(got, ref.want, ref.bound):.4f} | {s_ratio:.4f} | {ms:.2f}")
    print(line)
    log(line)
    assert n == 0, f"{name}: {n}/{got.numel()} elements outside the bound, worst {R.worst(got, ref, cs)}"
    if cs.o_fp8:          # the fp8 store rounds the fp16 value of the same launch
        b16, _ = launch(cs, dev, operands, fp8=False)
        g16, clean = split(cs, b16, False)
        assert clean and torch.equal(got, R.to_e4m3(g16)), f"{name}: the fp8 bytes are not E4M3 of the same launch's fp16 output"
    if cs.ident_from:
        r0 = cs.ident_from * cs.Tq
        V = R.to_o_layout(R.unpack(cs, host)[1][0][1][:, :, :cs.Tq].double())
        assert torch.equal(got[r0:], V[r0:]), f"{name}: identity rows are not V"
        plain, _ = launch(cs, dev, operands, batch=cs.ident_from, ident_from=0)
        gp, _ = split(cs, plain, False)
        assert torch.equal(gp[:r0], got[:r0]), f"{name}: attending rows differ from the launch without the identity rows"
        assert (gp[r0:] == R.SENTINEL).all()
