"""CPU: the fp64 reference and the derived interval of tests/xattn_ref.py mean something before any GPU runs.  The fp32 stand-in
of the to_q + cross-attention epilogue -- a correct kernel by construction -- lies inside [lo, hi] at every case with no element
left out; every mutant of it lies outside at the case `CAUGHT_AT` names; the reference without its rounding points is plain
softmax(q k^T) v summed over the segments; the case table reaches what it claims; the planted keys win by the stated margin on
the stored values."""
import math

import pytest
import torch

import gemm_conv_ref as G
import xattn_ref as X


@pytest.fixture(scope="module")
def refs():
    """name -> (operands, Ref): computed once, shared, never changed."""
    return {name: (X.operands(cs), X.reference(cs)) for name, cs in X.CASES.items()}


@pytest.mark.parametrize("name", list(X.CASES))
def test_standin_is_inside_the_interval(refs, name):
    cs = X.CASES[name]
    ops, ref = refs[name]
    got = X.standin(cs, ops)
    assert got.shape == ref.want.shape == (cs.R * cs.Tq, cs.heads * 64)
    assert torch.isfinite(ref.lo).all() and torch.isfinite(ref.hi).all() and (ref.lo <= ref.want).all() and (ref.want <= ref.hi).all()
    n, ratio = X.outside(got, ref)
    print(f"{name}: stand-in worst err/bound {ratio:.4f}, != want {int((got != ref.want).sum())} of {got.numel()}, "
          f"pinned elements (lo == hi) {int((ref.lo == ref.hi).sum())}")
    assert n == 0, f"{name}: {n}/{got.numel()} elements of the stand-in outside [lo, hi], worst {X.worst(got, ref, cs)}"


@pytest.mark.parametrize("mut", X.MUTANTS)
def test_mutant_is_outside_the_interval(refs, mut):
    name = X.CAUGHT_AT[mut]
    cs = X.CASES[name]
    ops, ref = refs[name]
    n, _ = X.outside(X.standin(cs, ops, mut), ref)
    print(f"{mut} at {name}: {n} elements outside")
    assert n > 0, f"{mut}: inside the interval at {name}"


def test_every_mutant_is_named():
    assert set(X.CAUGHT_AT) == set(X.MUTANTS) and set(X.CAUGHT_AT.values()) <= set(X.CASES)


@pytest.mark.parametrize("name", ["wg1.k64.t77_16", "k320.t80_1.fold4.plant", "k64.t17_16.big", "k64.t65_57.equal", "k128.t1_64.nobias.h4"])
def test_reference_without_rounding_is_plain_attention(name):
    """q = the unrounded projection (LayerNorm fold included), natural-base softmax of q k^T ln 2, times v, summed."""
    cs = X.CASES[name]
    ops = X.operands(cs)
    got = X.reference(cs, ops, rounding=False).want
    q = X.heads_of(G.reference("gemm", ops.spec).p, cs)
    want = 0
    for kview, rows, vt, vbs, tkv in ops.kv:
        for_b = []
        for b in range(cs.R):
            k = kview[b * rows:b * rows + tkv].double().reshape(tkv, cs.heads, 64).permute(1, 0, 2)
            v = vt[:, b * vbs:b * vbs + tkv].double().reshape(cs.heads, 64, tkv).permute(0, 2, 1)
            for_b.append(torch.softmax(q[b] @ k.transpose(-1, -2) * math.log(2.0), dim=-1) @ v)
        want = want + torch.stack(for_b)
    want = X.to_o_layout(want)
    assert torch.isfinite(got).all()
    assert float((got - want).abs().max()) <= 1e-11 * max(1.0, float(want.abs().max()))


def test_rounded_reference_differs_from_the_unrounded_one_by_roundings_only():
    """The rounding points move `value` by what fp16 roundings of q and P can: far below the fp16 step of the operands times
    the row's reach, and not by nothing."""
    cs = X.CASES["wg1.k64.t77_16"]
    a, b = X.reference(cs), X.reference(cs, rounding=False)
    d = float((a.value - b.value).abs().max())
    assert 0 < d < 2e-3


def test_case_table_reaches_what_it_claims():
    cs = list(X.CASES.values())
    assert {c.tk for c in cs} >= set(X.TK_PAIRS)
    assert X.TK_PAIRS == ((1, 1), (80, 64), (80, 1), (1, 64), (7, 9), (8, 8), (9, 7), (16, 17), (17, 16), (65, 57), (73, 63), (79, 4))
    assert {X.k_tiles(c) for c in cs} == {1, 2, 3, 5}                       # K = 64 (shorter than the ring), 128, 192, 320 (wraps off a multiple of 3)
    assert {X.tiles_per_image(c) for c in cs} == {1, 2}
    assert {X.head_tiles(c) for c in cs} == {1, 2, 3}                        # heads 2, 4 (N = 256), 6 (N = 384): hd0 > 0
    assert {(c.R, c.Tq) for c in cs} >= {(1, 64), (3, 64), (2, 128)}
    one = X.CASES["wg1.k64.t77_16"]
    assert (one.R, one.Tq, one.heads, one.K, one.tk) == (1, 64, 2, 64, (77, 16))
    assert {c.fold for c in cs} >= {0, 1, 4} and any(not c.bias for c in cs) and any(c.fold and not c.bias for c in cs)
    assert {c.regime for c in cs} == {"flat", "plant", "big", "equal"}
    assert any(c.out_scale == 0.5 for c in cs)
    assert all(c.R * c.Tq <= 256 and c.heads * 64 <= 384 and c.K <= 320 for c in cs)


def test_operand_layout_is_what_the_gpu_file_relies_on():
    """Views of wider buffers, the header's % 8 / 16-byte rules, NaN around K and V^T, +-1000 on the pad columns."""
    for cs in X.CASES.values():
        ops = X.operands(cs)
        a, w = ops.spec["a"], ops.spec["w"]
        assert a.stride(0) > cs.K and a.stride(0) % 8 == 0 and a.storage_offset() % 8 == 0 and w.is_contiguous() and w.storage_offset() % 8 == 0
        if cs.bias:
            assert ops.spec["bias"].storage_offset() % 8 == 0
        assert (ops.spec.get("ln_in") is not None) == bool(cs.fold)
        C = cs.heads * 64
        for kview, rows, vt, vbs, tkv in ops.kv:
            assert kview.stride(0) > C and kview.stride(0) % 8 == 0 and kview.storage_offset() % 8 == 0 and rows > tkv
            assert vt.stride(0) % 8 == 0 and vt.storage_offset() % 8 == 0 and vbs % 8 == 0 and vbs > X.roundup8(tkv) and vt.stride(0) > cs.R * vbs
            kbuf = torch.empty(0, dtype=torch.half).set_(kview.untyped_storage()).reshape(-1, kview.stride(0))
            assert torch.isnan(kbuf[:, :X.BORDER]).all() and torch.isnan(kbuf[:, X.BORDER + C:]).all()
            tpad = X.roundup8(tkv)
            for b in range(cs.R):
                assert torch.isfinite(kview[b * rows:b * rows + tkv]).all() and torch.isnan(kview[b * rows + tkv:(b + 1) * rows]).all()
                assert torch.isfinite(vt[:, b * vbs:b * vbs + tkv]).all()
                assert (vt[:, b * vbs + tkv:b * vbs + tpad].abs() == X.PAD_V).all()
                assert torch.isnan(vt[:, b * vbs + tpad:(b + 1) * vbs]).all()


def test_planted_margins_hold_after_rounding():
    n = 0
    for cs in X.CASES.values():
        if cs.regime != "plant":
            continue
        ops, ref = X.operands(cs), X.reference(cs)
        assert len(ops.plants) == 2 * sum(t > 1 for t in cs.tk)
        assert {(sg, key) for _, sg, key in ops.plants} == {(sg, k) for sg, t in enumerate(cs.tk) if t > 1 for k in (0, t - 1)}
        got = X.margins(cs, ops, ref.q)
        print(cs.name, [round(m, 1) for m in got])
        assert min(got) >= X.MARGIN
        # and with q anywhere in its admitted interval: the margin moves by at most twice the row's reach
        worst = X.margins(cs, ops, ref.q - ref.dq * torch.sign(ref.q))
        assert min(worst) >= X.MARGIN - 2.0
        n += len(got)
    assert n >= 8


def test_big_regime_has_large_scores_and_distant_maxima():
    cs = X.CASES["k64.t17_16.big"]
    ops, ref = X.operands(cs), X.reference(cs)
    qh = X.heads_of(ref.q, cs)
    (K0, _, _), (K1, _, _) = X._kv_heads(cs, ops.kv)
    s0, s1 = qh @ K0.transpose(-1, -2), qh @ K1.transpose(-1, -2)
    assert float(s0.abs().mean()) > 100 and float(s1.abs().mean()) > 100
    assert int(((s0.max(-1).values - s1.max(-1).values).abs() > 150).sum()) > 0


def test_equal_regime_is_the_mean_of_v():
    cs = X.CASES["k64.t65_57.equal"]
    ops = X.operands(cs)
    got = X.reference(cs, ops, rounding=False).want
    want = sum(V.mean(2, keepdim=True).expand(-1, -1, cs.Tq, -1) for _, V, _ in X._kv_heads(cs, ops.kv))
    assert float((got - X.to_o_layout(want)).abs().max()) < 1e-12


def test_gemm_reference_exposes_the_admitted_interval():
    """`gemm_conv_ref.Ref.lo / hi`: want inside, bound = the larger distance + tiny, as before."""
    ref = G.reference(*G.gemm_case("f16", "res", 64, 128, 64))
    assert (ref.lo <= ref.want).all() and (ref.want <= ref.hi).all()
    assert torch.equal(ref.bound, torch.maximum(ref.hi - ref.want, ref.want - ref.lo) + G.TINY[torch.float16])
