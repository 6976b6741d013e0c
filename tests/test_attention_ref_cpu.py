"""CPU: the fp64 attention reference and its bound (tests/attention_ref.py) checked without a GPU.

  * without its rounding points the reference is softmax(q k^T scale) v in float64, at every case of the GPU file;
  * the fp32 stand-ins of the two kernels -- correct by construction -- have 0 elements outside the bound at every one of them;
  * every mutant of a stand-in (one deliberate fault each) leaves the bound, and a mutant that cannot touch a case leaves the
    stand-in's bits alone there;
  * under `build_of` / `tiles_of` the case list reaches every build, every `attn_tile` instantiation and every rescale placement,
    the last read from the stand-in's own trace.
"""
import functools
import math

import pytest
import torch

import attention_ref as R

NAMES = list(R.CASES)


@functools.lru_cache(maxsize=None)
def ref_of(name):
    return R.reference(R.CASES[name])


@functools.lru_cache(maxsize=None)
def standin_of(name, mut=None):
    return R.standin(R.CASES[name], mut=mut)


@functools.lru_cache(maxsize=None)
def trace_of(name):
    tr = []
    R.standin(R.CASES[name], trace=tr)
    return tr


def _softmax_ref(cs):
    """torch.softmax in natural units, straight from the (B, Tq, C) / (B, Tkv, C) tensors the views hold."""
    q, segs = R.unpack(cs, R.operands(cs))
    nb = cs.ident_from or cs.B
    out = 0
    for K, Vp, Tkv in segs:
        s = q[:nb].double() @ K[:nb].double().transpose(-1, -2) * (math.log(2.0) if cs.qpre else cs.scale)
        if cs.causal:
            s = s.masked_fill(torch.ones(cs.Tq, Tkv, dtype=torch.bool).triu(1), -float("inf"))
        out = out + torch.softmax(s, dim=-1) @ Vp[:nb, :, :Tkv].double()
    return R.to_o_layout(out)


@pytest.mark.parametrize("name", NAMES)
def test_reference_without_rounding_points_is_softmax(name):
    cs = R.CASES[name]
    got = R.reference(cs, rounding=False).want
    want = _softmax_ref(cs)
    n = want.shape[0]
    assert torch.allclose(got[:n], want, rtol=1e-12, atol=1e-12), float((got[:n] - want).abs().max())


@pytest.mark.parametrize("name", NAMES)
def test_standin_is_inside_the_bound(name):
    cs, ref = R.CASES[name], ref_of(name)
    got = standin_of(name)
    n, ratio = R.compare(got, ref.want, ref.bound)
    print(f"{name}: build {R.build_of(cs)}, stand-in worst err / bound {ratio:.4f}, largest bound {float(ref.bound.max()):.3g}")
    assert n == 0, f"{n}/{got.numel()} elements of the stand-in outside the bound, worst {R.worst(got, ref, cs)}"
    assert (ref.lo <= ref.want).all() and (ref.want <= ref.hi).all()
    if cs.ident_from:
        assert (ref.bound[cs.ident_from * cs.Tq:] == 0).all()


# mutant -> the cases it must leave the bound at
MUT_OUT = {
    "ragged_off_by_one": ["pre.t7", "pre.t65", "pre.t200", "ring2.place.n1", "hd80.ragged.n1", "hd104.late.n8"],
    "causal_ge": ["ring2.causal77", "ring2.causal200.n8", "hd80.causal.n1"],
    "causal_gt1": ["ring2.causal77", "ring2.causal50x136", "ring3.causal77", "hd104.causal.n8"],
    "rise_o_only": ["pre.place.n1", "ring2.place.n8", "hd104.late.n1"],
    "rise_l_only": ["pre.place.n1", "ring2.place.n8", "hd80.late.n1"],
    "no_c1_fix": ["pre.place.n1", "ring2.place.n1", "ring2.causal200"],
    "no_pending_scale": ["pre.place.n1", "ring2.place.n1", "pre.mid"],
    "seg2_inherits": ["pre.2seg.77.64", "ring2.2seg.300.77", "hd80.2seg.n1"],
    "k_perm": ["pre.t64", "ring2.t257", "hd80.ragged.n1"],
    "no_log2e": ["pre.t64", "ring2.causal77", "hd80.ragged.n1"],
    "c_twice": ["pre.qpre", "ring2.causal.qpre", "hd80.qpre.n1"],
    "head_xor": ["pre.t64", "hd104.ragged.n1"],
    "batch0_vt": ["pre.t64", "ring2.t257", "hd80.ragged.n1"],
    "pad_col": ["pre.t7", "pre.t65", "ring2.t257", "hd80.ragged.n1"],
}
# mutant -> cases it cannot change: the stand-in's bits must stay as they are
MUT_SAME = {
    "causal_ge": ["pre.t64", "hd80.ragged.n1"],
    "causal_gt1": ["pre.place.n1"],
    "ragged_off_by_one": ["pre.t256", "ring2.t320"],          # no masked tile
    "pad_col": ["pre.t64", "pre.t200"],                         # Tkv % 8 == 0
    "c_twice": ["pre.t64", "hd80.ragged.n1"],                   # not pre-scaled
    "seg2_inherits": ["pre.t65", "hd80.ragged.n1"],
    "no_c1_fix": ["ring2.t320", "pre.t256"],                    # no masked tile
    "batch0_vt": ["grid1"],
    "fp8_from_fp32": ["pre.t64"],                               # fp16 output
}


@pytest.mark.parametrize("mut,name", [(m, n) for m, ns in MUT_OUT.items() for n in ns])
def test_mutant_leaves_the_bound(mut, name):
    ref = ref_of(name)
    n, ratio = R.compare(standin_of(name, mut), ref.want, ref.bound)
    assert R.compare(standin_of(name), ref.want, ref.bound)[0] == 0
    assert n > 0, f"mutant {mut} stays inside the bound at {name} (worst err / bound {ratio:.3f})"


@pytest.mark.parametrize("mut,name", [(m, n) for m, ns in MUT_SAME.items() for n in ns])
def test_mutant_that_cannot_touch_a_case_changes_nothing(mut, name):
    assert torch.equal(standin_of(name, mut), standin_of(name))
    ref = ref_of(name)
    assert R.compare(standin_of(name, mut), ref.want, ref.bound)[0] == 0


def test_every_mutant_is_exercised():
    assert set(MUT_OUT) | {"fp8_from_fp32"} == set(R.MUTANTS)


def test_fp8_store_from_fp32_is_seen_by_the_same_launch_in_fp16():
    """The fp8 store rounds the fp16 value.  A store that rounds the fp32 value differs from it only where the fp16 rounding lands on
    an E4M3 tie; the shift of the bound is never below half an fp16 ulp (u_P * A >= 2^-11 |value|), so the interval admits both E4M3
    neighbours there and cannot see this mutant.  What sees it is the GPU file's second assertion on every fp8 case: the bytes equal
    `to_e4m3` of the SAME launch's fp16 output.  Here: the two roundings differ somewhere on the fp8 cases, and that assertion
    fails for the mutant."""
    for name in ("pre.o_fp8", "pre.o_fp8.2seg.n8"):
        cs = R.CASES[name]
        o16 = R.standin(cs._replace(o_fp8=False))
        good, bad = standin_of(name), standin_of(name, "fp8_from_fp32")
        assert torch.equal(good, R.to_e4m3(o16))
        if name == "pre.o_fp8":
            assert not torch.equal(bad, R.to_e4m3(o16)), "the two roundings agree everywhere: the case does not separate them"
            assert int((bad != good).sum()) > 0


# ---- coverage -------------------------------------------------------------------------------------------------------------------------
def test_every_build_is_reached():
    builds = {R.build_of(c) for c in R.CASES.values()}
    assert builds == {"pre", "ring2", "ring3", "pre.ident", "ring2.ident", "ring3.ident", "hd80", "hd104"}, builds
    for b in ("pre", "ring2", "ring3", "hd80", "hd104"):          # two score regimes per build
        sigs = {c.sig for c in R.CASES.values() if R.build_of(c) == b}
        assert len(sigs) == 2, (b, sigs)
    assert {R.n_attending(c) for c in R.CASES.values()} >= {1, 7, 8, 9, 513, 520}
    assert any(c.causal for c in R.CASES.values() if R.build_of(c) == "ring3")
    assert any(len(c.tkvs) == 2 for c in R.CASES.values() if R.build_of(c) == "ring3")


def test_every_tile_instantiation_is_reached():
    for b in ("pre", "ring2", "ring3"):
        inst = {(f, m) for c in R.CASES.values() if R.build_of(c) == b for t in c.tkvs for _, f, m in R.tiles_of(c, t)}
        want = {(True, False), (True, True), (False, False), (False, True)}
        assert inst == want, (b, inst)


def _entry(tr, seg, tile, half):
    hit = [e for e in tr if (e["seg"], e["tile"], e["half"]) == (seg, tile, half)]
    assert len(hit) == 1, (seg, tile, half)
    return hit[0]


PLANTED = [n for n, c in R.CASES.items() if c.D == 64 and c.plants]


@pytest.mark.parametrize("name", PLANTED)
def test_planted_rescales_fire_where_planted(name):
    """From the stand-in's trace: at the (tile, half) of every planted key the wave's threshold test fires, the planted row's delta
    is what the plant's kind asks for, and another row of the same wave rides along with a delta below the threshold."""
    cs, tr = R.CASES[name], trace_of(name)
    for row, sg, key, kind in cs.plants:
        e = _entry(tr, sg, key // R.KT, "a" if key % R.KT < 32 else "b")
        d = e["delta"][:, :, row]
        assert e["fired"]
        lo = {"p": R.THR, "p2": R.THR, "huge": 150.0, "mid": 14.0}[kind]
        assert (d > lo).all(), (name, row, key, kind, float(d.min()))
        if kind == "mid":
            assert (d <= 24.0).all(), float(d.max())
            assert (torch.exp2(-d).half() < 2.0 ** -14).all()          # ah is an fp16 subnormal
        if kind == "huge":
            assert (torch.exp2(-d) == 0).all() and (torch.exp2(-d).half() == 0).all()          # alpha = 0, ah = 0
        w0 = row // 32 * 32
        riders = e["delta"][:, :, w0:min(w0 + 32, cs.Tq)]
        if riders.shape[-1] > 1:
            assert (riders <= R.THR).any(), "no row of the wave rides along"


def test_rescale_placements_are_reached_on_every_build():
    """FIRST tile half b; steady tile half a; steady tile half b; both halves of one tile; masked last tile half a and half b."""
    for name in ("pre.place.n1", "pre.place.n8", "ring2.place.n1", "ring2.place.n8", "ring3.place.n8"):
        cs = R.CASES[name]
        fired = {(e["first"], e["masked"], e["half"]) for e in trace_of(name) if e["fired"]}
        assert fired >= {(True, False, "b"), (False, False, "a"), (False, False, "b"), (False, True, "a"), (False, True, "b")}, (name, fired)
        a, b = _entry(trace_of(name), 0, 2, "a"), _entry(trace_of(name), 0, 2, "b")
        assert (a["delta"][:, :, 97] > R.THR).all() and (b["delta"][:, :, 97] > R.THR).all(), "both halves of tile 2, row 97"
        assert R.build_of(cs) == name.split(".")[0]
    fired = {(e["first"], e["masked"], e["half"]) for e in trace_of("ring2.causal200") if e["fired"]}
    assert fired >= {(True, True, "b"), (False, True, "a"), (False, True, "b")}, fired          # causal: every tile is a masked one
