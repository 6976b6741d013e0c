"""CPU: the fp64 reference of csrc/pointwise.hip, its bound, its stand-ins and its case table (tests/pointwise_ref.py) checked
without a GPU.

  * the restatement against what the project already trusts: the oracle's timestep embedding and `oracle/sched.py`'s `lcm_step`
    (both fp32: inside the fp32 slack the reference derives for the same operation count), `torch.std` in float64 for the
    rescale, a literal transcription of the reference's two blend loops, `F.silu` in float64;
  * every stand-in inside its bound at every case; for the bit classes lo == hi == stand-in wherever the slack does not cross a
    rounding boundary (the share of elements where it does is printed per entry, not asserted);
  * every mutant of a stand-in (one deliberate fault each) leaves the bound -- for the bit classes: changes bits -- at the cases
    named next to it;
  * the case table has every class the GPU file is meant to launch, so that a later edit cannot drop one;
  * the refusals of `instantir_amd/ops.py` for tensors that cannot hold what the launch would touch, each before any library call.
"""
import collections

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pointwise_ref as R

NAMES = list(R.CASES)
_crossing = collections.defaultdict(lambda: [0, 0])


def test_reference_sinusoid_is_the_oracles_timestep_embedding():
    from oracle import nets
    for name in ("sin.timestep", "sin.time_ids", "sin.192"):
        cs, t = R.CASES[name], R.build(name)
        o = cs.opt
        ref = R.reference(name)["out"]
        view = lambda a: R.like(R._sin_written(cs, t), torch.from_numpy(a)).numpy()
        want = nets.sinusoid(t["vals"].reshape(-1), o["dim"]).double().reshape(o["rows"], o["n_vals"] * o["dim"]).numpy()
        assert (np.abs(view(ref.value) - want) <= view(ref.slack)).all(), name           # the oracle is fp32 with the same operations


def test_reference_lcm_step_is_the_oracles():
    from oracle import sched
    name = "lcm.b3.r2.hw297.nchw"
    cs, t = R.CASES[name], dict(R.build(name))
    acp, ts = sched.make_alphas_cumprod(), 499
    a = acp[ts]
    c_skip, c_out = sched.lcm_scalings(torch.tensor([ts], dtype=torch.int64))
    t["coef"] = torch.tensor([float(torch.sqrt(1 - a)), float(torch.sqrt(a)), float(c_out[0].float()), float(c_skip[0].float())], dtype=torch.float32)
    o = cs.opt
    Rr, (H, W) = o["B"] * o["rep"], o["hw"]
    ref = R._r_lcm(cs, t)["out_nchw"]
    sample = t["x"].repeat(o["rep"], 1, 1, 1)
    eps = t["eps"].float().reshape(Rr, H, W, R.CH).permute(0, 3, 1, 2)
    want = sched.lcm_step(acp, eps, ts, sample).double().numpy()
    view = lambda x: R.like(t["out_nchw"], torch.from_numpy(x)).numpy()
    assert (np.abs(view(ref.value) - want) <= view(ref.slack)).all()


@pytest.mark.parametrize("name", [n for n in NAMES if R.CASES[n].kind == "rescale"])
def test_reference_rescale_is_torch_std_in_float64(name):
    cs, t = R.CASES[name], R.build(name)
    u, tt, pp = (torch.from_numpy(v) for v in R._rs_rows(cs, t, torch.float64))
    cfg = u + R.RS_G * (tt - u)
    if cs.opt["pag"]:
        cfg = cfg + cs.opt["pag"] * (tt - pp)
    phi = float(np.float32(cs.opt["phi"]))
    want = phi * tt.std(dim=(1, 2)) / cfg.std(dim=(1, 2)) + (1 - phi)
    ref = R.reference(name)["factor"]
    got = R.like(t["factor"], torch.from_numpy(ref.value))
    assert (torch.abs(got - want) <= 64 * R.U64 * want.abs()).all()                      # a few fp64 operations and two pairwise sums


@pytest.mark.parametrize("name", [n for n in NAMES if R.CASES[n].kind == "blend"])
def test_reference_blend_is_the_two_loops(name):
    """module/diffusers_vae/autoencoder_kl.py:311-321 transcribed; tiles of different size are cropped to the common extent first
    (the reference's slices need equal shapes; the clipping is the kernel's own convention, stated in csrc/pointwise.hip)."""
    o, t = R.CASES[name].opt, R.build(name)
    a, b = t["a"].double().clone(), t["b"].double().clone()
    ext = o["ext"]
    if o["vertical"]:
        w = min(a.shape[3], b.shape[3])
        av, bv = a[:, :, :, :w], b[:, :, :, :w]
        for y in range(ext):
            bv[:, :, y, :] = av[:, :, -ext + y, :] * (1 - y / ext) + bv[:, :, y, :] * (y / ext)
    else:
        h = min(a.shape[2], b.shape[2])
        av, bv = a[:, :, :h], b[:, :, :h]
        for x in range(ext):
            bv[:, :, :, x] = av[:, :, :, -ext + x] * (1 - x / ext) + bv[:, :, :, x] * (x / ext)
    got = R.like(t["b"], torch.from_numpy(R.reference(name)["b"].value))
    assert (torch.abs(got - b) <= 4 * R.U64 * b.abs()).all()


def test_reference_silu_is_torch_in_float64():
    for name in (n for n in NAMES if R.CASES[n].kind == "silu"):
        t = R.build(name)
        got = R.like(t["out"], torch.from_numpy(R.reference(name)["out"].value))
        want = F.silu(t["x"].double())
        assert (torch.abs(got - want) <= 4 * R.U64 * want.abs()).all()


@pytest.mark.parametrize("name", NAMES)
def test_standin_is_inside_the_bound(name):
    cs = R.CASES[name]
    ref, got = R.reference(name), R.standin(name)
    assert set(ref) == set(got)
    for out, r in ref.items():
        assert not np.isnan(r.want).any() and (r.lo <= r.want).all() and (r.want <= r.hi).all()
        g = R.as64(got[out])
        n, ratio = R.compare(g, r)
        print(f"{name}.{out}: stand-in worst err / bound {ratio:.3f}")
        assert n == 0, (name, out, R.worst(g, r))
        if cs.kind in R.BIT_KINDS:
            tight = r.lo == r.hi
            assert (g[tight] == r.lo[tight]).all()
            _crossing[cs.kind][0] += int((~tight).sum())
            _crossing[cs.kind][1] += tight.size


def test_share_of_elements_whose_slack_crosses_a_rounding_boundary():
    """Printed, not asserted (runs after the cases above)."""
    for kind, (n, tot) in _crossing.items():
        print(f"{kind}: lo != hi at {n} of {tot} elements ({100.0 * n / max(tot, 1):.2f} %)")


# mutant -> cases at which it must leave the bound (bit classes: and so change bits)
MUT = {
    "sin_cos_swapped": ["sin.one", "sin.192", "sin.timestep"],
    "sin_k_over_dim": ["sin.192", "sin.time_ids", "sin.270"],
    "silu_tail_dropped": ["silu.n8", "silu.n1000", "silu.n2056"],
    "ca_scale_index_m_plus_1": ["ca.rps1", "ca.rps35", "ca.c8", "ca.c2560"],
    "ca_add_scale_ignored": ["ca.rps1", "ca.rps35", "ca.rpsM", "ca.c2560"],
    "pack_row_b_rep_k": ["pack.2x4x5x7.r2.ld8.f16.s0862.host", "pack.3x4x16x17.r3.ld8.bf16.s0862.dev", "pack.2x4x5x7.r3.ld8.f16.big.dev"],
    "unpack_pixel_channel_swapped": ["unpack.2x4x5x7.ld8.f16", "unpack.3x4x16x17.ld8.bf16", "unpack.3x4x16x17.ld4.f16"],
    "rs_uncond_dev": ["rs.b1.hw35.plain.phi0.7", "rs.b3.hw1024.plain.phi0.7", "rs.b3.hw2211.pag2.75.phi0.7", "rs.b3.hw2211.plain.phi0.7.lm100"],
    "rs_pag_sign": ["rs.b3.hw2211.pag2.75.phi0.7", "rs.b1.hw35.pag2.75.phi1", "rs.b3.hw1025.pag2.75.phi1.lm100"],
    "rs_drop_p1024": ["rs.b3.hw1025.plain.phi1", "rs.b3.hw2211.plain.phi0.7", "rs.b3.hw2211.pag2.75.phi0.7", "rs.b3.hw2211.plain.phi0.7.lm100"],
    "lcm_image_r_div_rep": ["lcm.b2.r2.hw297.nchw", "lcm.b3.r2.hw35.nhwc", "lcm.b3.r2.hw297.nchw"],
    "tr_no_zero_fill": ["tr.77x64.p80", "tr.1x8.p8", "tr.33x33.p40", "tr.257x40.p264"],
    "tr_clamp_last_tile": ["tr.77x64.p80", "tr.33x33.p40", "tr.40x64.p48", "tr.257x40.p264"],
    "cs_max_units_for_every_job": ["seg.three", "seg.grid"],
    "bl_w_ext_minus_1": ["bl.v.same.e7", "bl.h.same.e7", "bl.v.wa_lt_wb.full", "bl.h.ha_lt_hb.full"],
    "bl_a_row_y": ["bl.v.same.e7", "bl.v.wa_gt_wb.e1"],                  # (ext = Ha: row Ha - ext + y IS row y)
    "bl_h_clip_hb": ["bl.h.ha_lt_hb.full", "bl.h.ha_lt_hb.e7"],
    "axpby_coef_swapped": ["axpby.n1", "axpby.n255", "axpby.n257", "axpby.n70"],
    "st_kh_kn_swapped": ["sh.n255.noise.x0.full", "sh.n257.noise.full"],
}
REQUIRED_MUTANTS = set(MUT) - {"silu_tail_dropped", "st_kh_kn_swapped"}                   # the 17 the table must never lose


def test_every_mutant_is_listed():
    have = {m for ms in R.MUTANTS.values() for m in ms}
    assert have == set(MUT) and REQUIRED_MUTANTS <= have and len(REQUIRED_MUTANTS) == 17
    for mut, names in MUT.items():
        assert names and all(n in R.CASES and mut in R.MUTANTS[R.CASES[n].kind] for n in names), mut


@pytest.mark.parametrize("mut,name", [(m, n) for m, names in MUT.items() for n in names])
def test_mutant_is_caught(mut, name):
    cs = R.CASES[name]
    ref, got, clean = R.reference(name), R.standin(name, mut), R.standin(name)
    outside = sum(R.compare(R.as64(got[o]), r)[0] for o, r in ref.items())
    print(f"{mut} at {name}: {outside} elements outside the bound")
    assert outside > 0, (mut, name)
    if cs.kind in R.BIT_KINDS:
        assert any(not np.array_equal(R.bits(got[o]), R.bits(clean[o])) for o in ref), (mut, name)


def test_case_table_has_every_class():
    by = collections.defaultdict(list)
    for c in R.CASES.values():
        by[c.kind].append(c.opt)
    some = lambda kind, f: any(f(o) for o in by[kind])
    # sinusoid: one thread, one partial block, more than one block without being a multiple of it, both engine forms, the values
    tot = lambda o: o["rows"] * o["n_vals"] * o["dim"] // 2
    assert some("sinusoid", lambda o: tot(o) == 1) and some("sinusoid", lambda o: tot(o) == 192)
    assert some("sinusoid", lambda o: tot(o) > 256 and tot(o) % 256)
    assert some("sinusoid", lambda o: (o["rows"], o["n_vals"], o["dim"]) == (3, 6, 256) and o["col_off"] > 0)
    assert some("sinusoid", lambda o: o["n_vals"] == 1 and o["dim"] == 320)
    vals = set()
    for n, c in R.CASES.items():
        if c.kind == "sinusoid":
            t = R.build(n)
            vals |= set(t["vals"].reshape(-1).tolist())
            o = c.opt
            assert o["col_off"] + o["n_vals"] * o["dim"] < t["out"].shape[1] < t["out"].stride(0)           # sentinel columns after, ldo wider
    assert {0.0, 1.0, 999.0, 1024.0} <= vals and any(v != int(v) for v in vals)
    assert some("sinusoid", lambda o: o["col_off"] > 0)
    # silu
    assert {o["n"] for o in by["silu"]} >= {8, 2048 + 8} and some("silu", lambda o: (o["n"] // 8) % 256 and o["n"] < 2048)
    x = R.build("silu.n2056")["x"].double()
    assert {65504.0, -65504.0} <= set(x.tolist()) and (x == 0).sum() == 2 and torch.signbit(x[x == 0]).sum() == 1
    assert ((x != 0) & (x.abs() < 2.0 ** -14)).any() and x.min() < -11.9 and x.max() > 11.9 and ((x > -12) & (x < 12)).sum() > 2000
    # copy_add
    assert some("copy_add", lambda o: not o["add"]) and some("copy_add", lambda o: o["add"] and not o["rps"])
    for rps in (1, 35):
        assert some("copy_add", lambda o: o["rps"] == rps)
    assert some("copy_add", lambda o: o["rps"] == o["M"]) and some("copy_add", lambda o: o["rps"] and o["M"] % o["rps"])
    assert {8, 2560} <= {o["C"] for o in by["copy_add"]}
    assert some("copy_add", lambda o: o["add"] and len({o["lds"], o["lda"], o["ldd"]}) == 3 and min(o["lds"], o["lda"], o["ldd"]) > o["C"])
    assert some("copy_add", lambda o: o["dst_off"] == 0) and some("copy_add", lambda o: o["dst_off"] > 0 and o["dst_off"] % 8 == 0)
    assert some("copy_add", lambda o: o["M"] * o["C"] // 8 > 256 and 256 % (o["C"] // 8))
    # pack / unpack
    for kind in ("pack", "unpack"):
        assert {o["shape"] for o in by[kind]} == {(1, 4, 1, 1), (2, 4, 5, 7), (3, 4, 16, 17)}
        assert {o["ld"] for o in by[kind]} == {4, 8} and {o["dtype"] for o in by[kind]} == {"f16", "bf16"}
    assert {o["rep"] for o in by["pack"]} == {1, 2, 3} and {o["scale"] for o in by["pack"]} == {"s1", "s0862", "big"}
    assert {o["dscale"] for o in by["pack"]} == {True, False}
    big = R.reference("pack.3x4x16x17.r3.ld4.f16.big.host")["out"].want
    assert np.isinf(big).any() and ((big != 0) & (np.abs(big) < 2.0 ** -14)).any()
    for n, c in R.CASES.items():
        if c.kind == "unpack" and c.opt["ld"] > R.CH:
            assert torch.isnan(R.flat(R.build(n)["x"]).reshape(-1, c.opt["ld"])[1:-1, R.CH:]).all()
    # cfg_rescale
    rs = by["rescale"]
    assert {o["B"] for o in rs} == {1, 3} and {35, 1024, 1025} <= {o["hw"][0] * o["hw"][1] for o in rs}
    assert any(o["hw"][0] * o["hw"][1] > 2048 and (o["hw"][0] * o["hw"][1]) % 64 for o in rs)
    assert {o["pag"] for o in rs} >= {None, 0.0, 2.75} and {o["phi"] for o in rs} >= {0.0, 0.7, 1.0} and {"lm100"} <= {o["mode"] for o in rs}
    assert R.RS_LDE == 8 and R.CH == 4
    for n, c in R.CASES.items():
        if c.kind == "rescale":
            e = R.flat(R.build(n)["eps"]).reshape(-1, R.RS_LDE)[1:-1]
            assert torch.isnan(e[:, R.CH:]).all()
            third = e[2 * e.shape[0] // 3:, :R.CH]
            assert torch.isnan(third).all() == (not c.opt["pag"])
    assert R.reference("rs.b3.hw2211.plain.phi0.7.lm100")["factor"].terms["mean_over_spread"] > 80
    # lcm_step
    assert {(o["B"], o["rep"]) for o in by["lcm"]} >= {(2, 1), (2, 2), (3, 1), (3, 2)} and {o["nchw"] for o in by["lcm"]} == {True, False}
    assert all(o["lde"] != o["ldo"] and min(o["lde"], o["ldo"]) > R.CH and (o["hw"][0] * o["hw"][1]) % 2 for o in by["lcm"])
    x = R.build("lcm.b3.r2.hw297.nchw")["x"]
    assert not torch.equal(x[0], x[1]) and not torch.equal(x[1], x[2])
    # transpose
    assert {o["shape"] for o in by["transpose"]} == {(77, 64, 80), (1, 8, 8), (33, 33, 40), (32, 32, 32), (40, 64, 48), (257, 40, 264)}
    t = R.build("tr.77x64.p80")
    assert t["x"].stride(0) > 64 and t["x"].storage_offset() % t["x"].stride(0) and t["out"].stride(0) > 80 and t["out"].storage_offset() % t["out"].stride(0)
    # copy_segments
    assert {o["units"] for o in by["segments"]} >= {(1,), (1, 4097, 300)}
    assert some("segments", lambda o: max(o["units"]) >= 256 * 1024 and min(o["units"]) == 5)
    # blend
    bl = by["blend"]
    assert {o["vertical"] for o in bl} == {True, False} and {o["ext"] for o in bl} >= {1, 7}
    assert any(o["vertical"] and o["Wa"] > o["Wb"] for o in bl) and any(o["vertical"] and o["Wa"] < o["Wb"] for o in bl)
    assert any(not o["vertical"] and o["Ha"] > o["Hb"] for o in bl) and any(not o["vertical"] and o["Ha"] < o["Hb"] for o in bl)
    assert any(o["vertical"] and o["ext"] == min(o["Ha"], o["Hb"]) for o in bl) and any(not o["vertical"] and o["ext"] == min(o["Wa"], o["Wb"]) for o in bl)
    assert R.BLEND_PLANES[0] * R.BLEND_PLANES[1] == 6
    # axpby and the fp32 steps
    assert {o["n"] for o in by["axpby"]} == {1, 255, 257, 70}
    for hist in (False, True):
        st = [o for o in by["step"] if o["hist"] == hist]
        assert {o["n"] for o in st} == {1, 255, 257, 70}
        assert {o["noise"] for o in st} == {True, False} and {o["x0"] for o in st} == {True, False}
        assert any(o["coef"] == "zero" and o["noise"] for o in st)
    z = R.build("sh.n257.noise.x0.zero")
    assert torch.isnan(z["noise"]).all() and torch.isnan(z["hist"]).all() and (z["coef"][5:] == 0).all()
    # prefetch
    assert set(R.PREFETCH_CASES) == {(100, 1), (100, 32), (128 * 1000 + 60, 1), (128 * 1000 + 60, 32)}


# ---- the refusals of ops.py ---------------------------------------------------------------------------------------------------------
class _Reached(Exception):
    pass


@pytest.fixture
def ops(monkeypatch):
    """`ops` with the CUDA requirement of `_chk2d` lifted and a library that only reports that it was reached: a refusal must
    come before `lib.load()`, and an operand set that fits must get that far."""
    from instantir_amd import ops as O

    def chk2d(t, name, dtype=torch.float16):
        if t.dtype != dtype or t.dim() != 2 or t.stride(1) != 1:
            raise ValueError(f"{name}: expected a 2-D {dtype} tensor with unit column stride")

    def load():
        raise _Reached()

    monkeypatch.setattr(O, "_chk2d", chk2d)
    monkeypatch.setattr(O.L, "load", load)
    monkeypatch.setattr(O, "_stream", lambda: 0)
    return O


def _refused(fn, *a, **k):
    with pytest.raises(ValueError):
        fn(*a, **k)


def _fits(fn, *a, **k):
    with pytest.raises(_Reached):
        fn(*a, **k)


def test_ops_refuse_what_the_tensors_cannot_hold(ops):
    h = lambda *s: torch.zeros(*s, dtype=torch.float16)
    f = lambda *s: torch.zeros(*s, dtype=torch.float32)
    # copy_add
    _fits(ops.copy_add, h(6, 16), h(6, 40), 24, add=h(6, 16), add_scale=f(2), rows_per_scale=3)
    _refused(ops.copy_add, h(6, 16), h(6, 39), 24)                                   # dst_off + C past the row
    _refused(ops.copy_add, h(6, 16), h(5, 40), 24)                                   # fewer rows than src
    _refused(ops.copy_add, h(6, 16), h(6, 40), 0, add=h(5, 16))
    _refused(ops.copy_add, h(6, 16), h(6, 40), 0, add=h(6, 24))
    _refused(ops.copy_add, h(6, 16), h(6, 40), 0, add=f(6, 16))
    _refused(ops.copy_add, h(6, 16), h(6, 40), 0, add=h(6, 16), add_scale=f(1), rows_per_scale=3)       # ceil(6 / 3) = 2 scales
    _refused(ops.copy_add, h(7, 16), h(7, 40), 0, add=h(7, 16), add_scale=f(2), rows_per_scale=3)       # ceil(7 / 3) = 3
    _refused(ops.copy_add, h(6, 16), h(6, 40), 0, add=h(6, 16), add_scale=h(2), rows_per_scale=3)
    _refused(ops.copy_add, h(6, 32)[:, ::2], h(6, 40), 0)
    # sinusoid
    _fits(ops.sinusoid, f(2, 3), h(2, 8 + 3 * 64), 64, col_off=8)
    _refused(ops.sinusoid, f(2, 3), h(2, 8 + 3 * 64 - 1), 64, col_off=8)
    _refused(ops.sinusoid, f(2, 3), h(1, 8 + 3 * 64), 64, col_off=8)
    _refused(ops.sinusoid, f(3, 2).T, h(2, 200), 64, col_off=8)
    _refused(ops.sinusoid, h(2, 3), h(2, 200), 64, col_off=8)
    # silu
    _fits(ops.silu, h(4, 16), h(4, 16))
    _refused(ops.silu, h(4, 16), h(4, 8))
    _refused(ops.silu, h(4, 16), f(4, 16))
    _refused(ops.silu, h(4, 32)[:, :16], h(4, 16))
    # pack / unpack
    _fits(ops.pack_latent, f(2, 4, 3, 5), h(2 * 2 * 15, 8), rep=2)
    _refused(ops.pack_latent, f(2, 4, 3, 5), h(2 * 15, 8), rep=2)
    _refused(ops.pack_latent, f(2, 4, 3, 5), h(60, 3), rep=2)
    _refused(ops.pack_latent, f(2, 4, 3, 5), h(61, 8), rep=2)
    _fits(ops.unpack_latent, h(30, 8), f(2, 4, 3, 5))
    _refused(ops.unpack_latent, h(29, 8), f(2, 4, 3, 5))
    _refused(ops.unpack_latent, h(30, 3), f(2, 4, 3, 5))
    # lcm_step
    _fits(ops.lcm_step, h(60, 8), 2, 2, f(4), f(2, 4, 3, 5), h(60, 16), f(4, 4, 3, 5))
    _fits(ops.lcm_step, h(60, 8), 2, 2, f(4), f(2, 4, 3, 5), h(60, 16))
    _refused(ops.lcm_step, h(30, 8), 2, 2, f(4), f(2, 4, 3, 5), h(60, 16))
    _refused(ops.lcm_step, h(60, 8), 2, 2, f(4), f(2, 4, 3, 5), h(30, 16))
    _refused(ops.lcm_step, h(60, 8), 2, 2, f(4), f(2, 4, 3, 5), h(60, 16), f(2, 4, 3, 5))
    _refused(ops.lcm_step, h(60, 8), 2, 2, f(4), f(4, 4, 3, 5), h(60, 16))           # x holds B images, not rep * B
    # transpose
    _fits(ops.transpose, h(77, 64), h(64, 160)[:, 80:], 80)
    _refused(ops.transpose, h(77, 64), h(63, 80), 80)
    _refused(ops.transpose, h(77, 64), h(64, 79), 80)
    _refused(ops.transpose, h(77, 64), h(64, 80), 76)
    # blend_tiles
    _fits(ops.blend_tiles, f(2, 3, 8, 8), f(1, 6, 8, 8), 4, True)
    _refused(ops.blend_tiles, f(2, 3, 8, 8), f(1, 5, 8, 8), 4, True)


def test_library_refuses_its_own_arguments_without_a_gpu():
    """What stays with the C entries (they validate before any HIP call): null pointers, non-positive sizes, strides below C."""
    from instantir_amd import lib
    h = lib.load()
    buf = torch.zeros(64, dtype=torch.float32)
    p = buf.data_ptr()
    for rc in (h.iir_lcm_step(p, 2, 1, 1, 4, 5, p, p, p, 8, None, None),          # lde < C
               h.iir_lcm_step(p, 8, 1, 0, 4, 5, p, p, p, 8, None, None),          # rep = 0
               h.iir_transpose_f16(p, 8, 4, 8, p, 8, 3, None),                    # rows_pad < rows
               h.iir_transpose_f16(p, 8, 4, 8, p, 7, 8, None),                    # ldo < rows_pad
               h.iir_copy_segments(p, 0, 1, None), h.iir_copy_segments(p, 1, 0, None),
               h.iir_prefetch(p, 0, 1, None), h.iir_prefetch(p, 128, 0, None),
               h.iir_blend_tiles_f32(p, p, 1, 4, 4, 4, 4, 5, 1, None),            # extent past the tile
               h.iir_axpby_f32(p, p, p, 0, p, None), h.iir_silu_f16(p, p, 12, None),
               h.iir_unpack_latent_t(p, 3, 1, 4, 5, p, 0, None), h.iir_pack_latent_t(p, 1, 4, 5, p, 3, 1, 1.0, 0, None)):
        assert rc != 0
