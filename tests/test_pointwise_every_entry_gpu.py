"""GPU: every exported entry of csrc/pointwise.hip but the descriptor step, the APG kernels and the timing entries, element by
element against the fp64 reference and the derived bound of tests/pointwise_ref.py (no tolerance: see that module's docstring), at
the smallest shapes at which each kernel's index arithmetic can still go wrong.  Every entry is launched through its `ops` wrapper
(`iir_pack_latent` / `iir_unpack_latent` are the fp16 spellings of the `_t` entries and share their launchers).

Every operand is a view of a wider buffer of its own (`on_dev`, as in tests/test_gemm_conv_every_build_gpu.py: the whole storage
goes to the device and the view keeps its strides and offset); inputs have NaN in the spare rows and columns, outputs a constant.
Per case and output tensor, over the WHOLE storage and leaving out no element:
  1. every written element lies in [lo, hi] and every other element keeps the bits it had;
  2. for the entries without a transcendental (`pointwise_ref.BIT_KINDS`) the storage equals the fp32 stand-in bit for bit.
Each launch runs twice on fresh buffers and both runs must agree in every bit.  Per entry the file prints, and appends to
profiles/pointwise_every_entry.log, the worst error / bound, the share of elements that differ from `want` and, for the bit
classes, the number of elements that differ from the stand-in.  tests/test_pointwise_ref_cpu.py shows that the stand-ins stay
inside the bound at these cases, that the mutants do not, and what the case table holds."""
import collections
import os
import time

import numpy as np
import pytest
import torch

import pointwise_ref as R

pytestmark = pytest.mark.gpu

LOG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "pointwise_every_entry.log")
_tally = collections.OrderedDict()


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from instantir_amd import lib
    lib.load()          # fails loudly if the HIP library is missing
    t0 = time.perf_counter()
    yield torch.device("cuda:0")
    lines = ["# entry | cases | elements | worst err/bound | share of elements != want | elements != stand-in (bit classes)"]
    for kind, (cases, n, ratio, neq, nbits) in _tally.items():
        lines.append(f"{kind} | {cases} | {n} | {ratio:.4f} | {neq / max(n, 1):.4f} | {nbits if kind in R.BIT_KINDS else '-'}")
    lines.append(f"# wall time of the file: {time.perf_counter() - t0:.1f} s")
    print("\n".join(lines))
    try:          # (a read-only checkout keeps the test, not the log)
        with open(LOG, "w") as f:
            f.write("\n".join(lines) + "\n")
    except OSError:
        pass


def on_dev(t, dev):
    """The same view of a device copy of t's whole storage (strides, offset and the bytes around the view kept)."""
    return R.like(t, R.flat(t).to(dev))


def _launch(cs, d, dev):
    from instantir_amd import ops
    o, k = cs.opt, cs.kind
    if k == "sinusoid":
        ops.sinusoid(d["vals"], d["out"], o["dim"], col_off=o["col_off"])
    elif k == "silu":
        ops.silu(d["x"], d["out"])
    elif k == "copy_add":
        ops.copy_add(d["src"], d["dst"], o["dst_off"], add=d.get("add"), add_scale=d.get("scale"), rows_per_scale=o["rps"] or 1)
    elif k == "pack":
        ops.pack_latent(d["x"], d["out"], rep=o["rep"], scale=d["scale"] if o["dscale"] else float(d["scale"].cpu()[0]))
    elif k == "unpack":
        ops.unpack_latent(d["x"], d["out"])
    elif k == "rescale":
        ops.cfg_rescale_factor(d["eps"][:, :R.CH], o["B"], d["coef"], d["x"], o["phi"], d["factor"], pag_scale=d.get("pag_s"))
    elif k == "lcm":
        ops.lcm_step(d["eps"], o["B"], o["rep"], d["coef"], d["x"], d["out"], d.get("out_nchw"))
    elif k == "transpose":
        ops.transpose(d["x"], d["out"], o["shape"][2])
    elif k == "segments":
        n = len(o["units"])
        table = ops.segment_job_table([(d[f"src{j}"], d[f"dst{j}"]) for j in range(n)], dev)
        assert table[2] == max(o["units"])
        ops.copy_segments(*table)
    elif k == "blend":
        ops.blend_tiles(d["a"], d["b"], o["ext"], o["vertical"])
    elif k == "axpby":
        ops.axpby_f32(d["x"], d["y"], d["coef"], d["out"])
    elif k == "step":
        ops.sched_step_f32(d["eps"], d["x"], d["coef"], d["prev"], noise=d.get("noise"), x0_out=d.get("x0_out"), hist=d.get("hist"))
    else:
        raise AssertionError(k)
    torch.cuda.synchronize()


def run(name, dev):
    """One launch of the case on fresh device copies: {output: its whole storage, on the CPU}, and the inputs' storages."""
    cs = R.CASES[name]
    d = {k: on_dev(v, dev) for k, v in R.build(name).items()}
    _launch(cs, d, dev)
    return {k: R.flat(v).cpu() for k, v in d.items()}


@pytest.mark.parametrize("name", list(R.CASES))
def test_entry(dev, name):
    cs = R.CASES[name]
    ref, want_bits, host = R.reference(name), R.standin(name), R.build(name)
    got, again = run(name, dev), run(name, dev)
    tally = _tally.setdefault(cs.kind, [0, 0, 0.0, 0, 0])
    tally[0] += 1
    fails = []
    for key, t in host.items():
        if key not in ref:          # an input: the launch may not have changed a bit of its storage
            assert np.array_equal(R.bits(got[key]), R.bits(R.flat(t))), f"{name}: input {key} changed"
    for out, r in ref.items():
        g = R.as64(got[out])
        n, ratio = R.compare(g, r)
        neq = int((g != r.want).sum())
        nbits = int((R.bits(got[out]) != R.bits(want_bits[out])).sum())
        tally[1] += g.size
        tally[2] = max(tally[2], ratio)
        tally[3] += neq
        tally[4] += nbits
        print(f"{name}.{out} | {g.size} | err/bound {ratio:.4f} | != want {neq} | != stand-in {nbits}")
        if n:
            fails.append(f"{out}: {n}/{g.size} elements outside the bound or the frame, first {R.worst(g, r)}")
        if cs.kind in R.BIT_KINDS and nbits:
            i = int(np.flatnonzero(R.bits(got[out]) != R.bits(want_bits[out]))[0])
            fails.append(f"{out}: {nbits} elements differ from the stand-in's bits, first at {i}: got {g[i]!r}, stand-in {R.as64(want_bits[out])[i]!r}")
        if not np.array_equal(R.bits(got[out]), R.bits(again[out])):
            fails.append(f"{out}: two runs differ")
    assert not fails, f"{name}: " + "; ".join(fails)


def test_device_and_host_scale_pack_the_same_bits(dev):
    a, b = run("pack.2x4x5x7.r2.ld8.f16.s0862.host", dev), run("pack.2x4x5x7.r2.ld8.f16.s0862.dev", dev)
    assert np.array_equal(R.bits(a["out"]), R.bits(b["out"]))


def test_pag_scale_zero_is_the_plain_launch(dev):
    a, b = run("rs.b3.hw2211.plain.phi0.7", dev), run("rs.b3.hw2211.pag0.phi0.7", dev)
    assert np.array_equal(R.bits(a["factor"]), R.bits(b["factor"]))


@pytest.mark.parametrize("nbytes,blocks", R.PREFETCH_CASES)
def test_prefetch(dev, nbytes, blocks):
    """iir_prefetch has no output: this shows an OK status, an unchanged range and an unchanged frame around it, no more --
    neither that a line was touched nor that none beyond the range was read."""
    from instantir_amd import ops
    g = torch.Generator().manual_seed(nbytes + blocks)
    host = torch.randint(0, 256, (nbytes + 512,), dtype=torch.uint8, generator=g)
    buf = host.to(dev)
    for _ in range(2):
        ops.prefetch(buf.data_ptr() + 256, nbytes, blocks)
    torch.cuda.synchronize()
    assert torch.equal(buf.cpu(), host)
