"""CPU: the LPIPS contract (tests/lpips_ref.py) against a closed form, its properties, the two weight formats, and every
refusal of instantir_amd.lpips / the new ops / the new C entries / the new CLI flags that happens before a launch."""
import ctypes

import numpy as np
import pytest
import torch

import lpips_ref as R
from instantir_amd import lib
from instantir_amd import lpips as LP


def _identity_net():
    """Width (8, 8, 8, 8, 8); every conv passes its first three channels through the centre tap, zero bias; lin weights 1."""
    convs, cin = [], 3
    for _ in range(13):
        w = torch.zeros(8, cin, 3, 3)
        for c in range(3):
            w[c, c, 1, 1] = 1.0
        convs.append((w, torch.zeros(8)))
        cin = 8
    return convs, [torch.ones(8) for _ in range(5)]


def _closed_form(a, b):
    """LPIPS of the identity net with plain numpy: tap l is the ReLU of the l-times max-pooled scaled image."""
    shift, scale = np.array(R.SHIFT).reshape(3, 1, 1), np.array(R.SCALE).reshape(3, 1, 1)
    ta, tb = (np.maximum(((2.0 * x.astype(np.float64) - 1.0) - shift) / scale, 0.0) for x in (a, b))
    terms = []
    for _ in range(5):
        na, nb = (t / (np.sqrt((t * t).sum(0, keepdims=True)) + 1e-10) for t in (ta, tb))
        terms.append(((na - nb) ** 2).sum(0).mean())
        h, w = ta.shape[1] // 2, ta.shape[2] // 2
        ta, tb = (t[:, :2 * h, :2 * w].reshape(3, h, 2, w, 2).max(axis=(2, 4)) for t in (ta, tb))
    return np.array(terms)


def test_identity_net_equals_the_closed_form():
    rng = np.random.default_rng(0)
    convs, lins = _identity_net()
    for H, W in ((16, 16), (37, 53), (17, 32)):
        a, b = rng.random((3, H, W)), rng.random((3, H, W))
        D, maps = R.lpips(torch.from_numpy(a)[None], torch.from_numpy(b)[None], convs, lins)
        want = _closed_form(a, b)
        assert np.abs(D[0].numpy() - want).max() <= 1e-12
        assert [tuple(m.shape[1:]) for m in maps] == [(H >> l, W >> l) for l in range(5)]


def _small_net(seed=5):
    convs, lins, shift, scale = LP.parse_state_dict(LP.synthetic_state_dict(seed, (8, 8, 16, 16, 8)))
    assert shift == R.SHIFT and scale == R.SCALE
    return convs, lins


def test_properties():
    g = torch.Generator().manual_seed(1)
    convs, lins = _small_net()
    a, b = torch.rand(2, 3, 19, 16, generator=g), torch.rand(2, 3, 19, 16, generator=g)
    Dab, _ = R.lpips(a, b, convs, lins)
    Dba, _ = R.lpips(b, a, convs, lins)
    Daa, _ = R.lpips(a, a, convs, lins)
    assert torch.equal(Daa, torch.zeros(2, 5, dtype=torch.float64))
    assert torch.equal(Dab, Dba) and bool((Dab > 0).all())
    for st in (torch.float16, torch.bfloat16):
        Ds, _ = R.lpips(a, b, convs, lins, storage=st)
        assert 0 < (Ds - Dab).abs().max() < 0.05 * Dab.max()
    # a pixel whose channels are all zero (x = 0 is below every shift: the ReLU of the identity net leaves nothing) gives 0, not NaN
    iconvs, ilins = _identity_net()
    z = torch.zeros(1, 3, 16, 16)
    Dz, mz = R.lpips(z, z, iconvs, ilins)
    assert torch.equal(Dz, torch.zeros(1, 5, dtype=torch.float64)) and all(bool((m == 0).all()) for m in mz)
    Dzb, _ = R.lpips(z, b[:1, :, :16], iconvs, ilins)
    assert bool(torch.isfinite(Dzb).all()) and bool((Dzb > 0).all())


def test_odd_size_is_scored_in_the_tap_and_dropped_by_the_pool():
    g = torch.Generator().manual_seed(2)
    convs, lins = _identity_net()
    a, b = torch.rand(1, 3, 17, 19, generator=g), torch.rand(1, 3, 17, 19, generator=g)
    D, maps = R.lpips(a, b, convs, lins)
    assert tuple(maps[0].shape) == (1, 17, 19) and tuple(maps[1].shape) == (1, 8, 9)
    a2 = a.clone()
    a2[:, :, 16, :] = 1.0 - a2[:, :, 16, :]              # the last row: in the first tap, in no pooled quad
    a2[:, :, :, 18] = 1.0 - a2[:, :, :, 18]
    D2, maps2 = R.lpips(a2, b, convs, lins)
    assert D2[0, 0] != D[0, 0] and torch.equal(D2[0, 1:], D[0, 1:])
    assert torch.equal(maps2[0][:, :16, :18], maps[0][:, :16, :18]) and not torch.equal(maps2[0][:, 16], maps[0][:, 16])


# ---- the weight formats ------------------------------------------------------------------------------------------------------
def _two_formats(tmp_path, widths=(8, 16, 16, 24, 8), scaling=False):
    whole = LP.synthetic_state_dict(9, widths)
    tv, lin = {}, {}
    for k, v in whole.items():
        if k.startswith("net.slice"):
            tv["features." + k.split(".", 2)[2]] = v
        else:
            lin[k] = v
    tv["classifier.0.weight"] = torch.zeros(4, 4)                         # what a torchvision file also holds
    for l in range(5):                                                      # the duplicates a whole lpips.LPIPS state dict carries
        whole[f"lins.{l}.model.1.weight"] = whole[f"lin{l}.model.1.weight"].clone()
    if scaling:
        whole["scaling_layer.shift"] = torch.tensor(R.SHIFT).view(1, 3, 1, 1)
        whole["scaling_layer.scale"] = torch.tensor(R.SCALE).view(1, 3, 1, 1)
    paths = [str(tmp_path / n) for n in ("vgg16.pth", "vgg_lin.pth", "lpips_whole.pth")]
    for p, sd in zip(paths, (tv, lin, whole)):
        torch.save(sd, p)
    return paths, whole


def test_both_formats_load_to_equal_tensors(tmp_path):
    (tv, lin, whole), sd = _two_formats(tmp_path)
    ca, la, sha, sca = LP.load_weights(tv, lin)
    cb, lb, shb, scb = LP.load_weights(whole)
    assert len(ca) == len(cb) == 13 and len(la) == len(lb) == 5
    assert all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(ca, cb))
    assert all(torch.equal(x, y) and x.dim() == 1 for x, y in zip(la, lb))
    assert [w.shape[0] for w, _ in ca] == [8, 8, 16, 16, 16, 16, 16, 24, 24, 24, 8, 8, 8]
    assert sha == shb == R.SHIFT and sca == scb == R.SCALE                # a file without scaling_layer.* gets LPIPS's constants
    (_, _, whole2), _ = _two_formats(tmp_path, scaling=True)
    _, _, sh2, sc2 = LP.load_weights(whole2)
    assert np.allclose(sh2, R.SHIFT, rtol=1e-7) and np.allclose(sc2, R.SCALE, rtol=1e-7)
    m = LP.LPIPS.from_files(whole, device="cpu")
    assert m.widths == (8, 16, 16, 24, 8) and m.padded == (64,) * 5
    assert tuple(m.w[0][0].shape) == (64, 3, 3, 64) and m.w[0][0].dtype == torch.float16 and float(m.w[0][0][8:].abs().max()) == 0.0


def test_loader_refusals_name_the_key(tmp_path):
    sd = LP.synthetic_state_dict(9, (8, 8, 8, 8, 8))
    bad = dict(sd)
    del bad["net.slice3.12.bias"]
    with pytest.raises(ValueError, match=r"missing key net\.slice3\.12\.bias"):
        LP.parse_state_dict(bad)
    bad = dict(sd)
    del bad["lin4.model.1.weight"]
    with pytest.raises(ValueError, match=r"missing key lin4\.model\.1\.weight"):
        LP.parse_state_dict(bad)
    bad = dict(sd)
    bad["net.slice2.7.weight"] = torch.zeros(8, 8, 5, 5)
    with pytest.raises(ValueError, match=r"net\.slice2\.7\.weight must be a \(Cout, Cin, 3, 3\) kernel"):
        LP.parse_state_dict(bad)
    bad = dict(sd)
    bad["net.slice1.0.weight"], bad["net.slice1.0.bias"] = torch.zeros(12, 3, 3, 3), torch.zeros(12)
    with pytest.raises(ValueError, match=r"net\.slice1\.0\.weight has 12 output channels"):
        LP.parse_state_dict(bad)
    bad = dict(sd)
    bad["lin2.model.1.weight"] = torch.zeros(1, 16, 1, 1)
    with pytest.raises(ValueError, match=r"lin2\.model\.1\.weight must be shaped \(1, 8, 1, 1\)"):
        LP.parse_state_dict(bad)
    tv = {"features." + k.split(".", 2)[2]: v for k, v in sd.items() if k.startswith("net.slice")}
    with pytest.raises(ValueError, match="needs the lin layers"):
        LP.parse_state_dict(tv)
    with pytest.raises(ValueError, match=r"missing key features\.28\.weight"):
        LP.parse_state_dict({k: v for k, v in tv.items() if k != "features.28.weight"}, {k: v for k, v in sd.items() if k.startswith("lin")})
    with pytest.raises(ValueError, match="five positive multiples of 8"):
        LP.synthetic_state_dict(1, (8, 8, 8, 12, 8))


# ---- refusals before any launch ----------------------------------------------------------------------------------------------
def test_module_refusals():
    m = LP.LPIPS.synthetic(3, (8, 8, 8, 8, 8), device="cpu")
    ok = torch.zeros(1, 3, 16, 16)
    with pytest.raises(ValueError, match="smallest side is 16"):
        m(torch.zeros(1, 3, 15, 40), torch.zeros(1, 3, 15, 40))
    with pytest.raises(ValueError, match="smallest side is 16"):
        m(torch.zeros(3, 64, 12), torch.zeros(3, 64, 12))
    with pytest.raises(ValueError, match="but its counterpart"):
        m(ok, torch.zeros(1, 3, 16, 17))
    with pytest.raises(ValueError, match="3 channels"):
        m(torch.zeros(1, 1, 16, 16), torch.zeros(1, 1, 16, 16))
    with pytest.raises(ValueError, match="a: expected"):
        m("a.png", ok)
    with pytest.raises(ValueError, match="no host path"):
        m(ok, ok)
    with pytest.raises(ValueError, match="dtype must be"):
        LP.LPIPS.synthetic(3, (8, 8, 8, 8, 8), device="cpu", dtype=torch.float32)
    # the 2 GiB rule: both images at full resolution in the first slice's 64 channels, 2 bytes each
    full = LP.LPIPS.synthetic(3, (64, 8, 8, 8, 8), device="cpu")
    full._check_geometry(2048, 2048)
    assert full._largest_activation_bytes(2048, 2048) == 1 << 30
    with pytest.raises(ValueError, match=r"largest activation \(2147483648 bytes\) reaches 2 GiB"):
        full._check_geometry(4096, 2048)
    from instantir_amd import metrics as M
    with pytest.raises(ValueError, match="smallest side"):
        M.lpips(torch.zeros(3, 8, 8), torch.zeros(3, 8, 8), m)
    assert M.METRICS == ("psnr", "ssim")


def test_ops_wrapper_refusals():
    from instantir_amd import ops
    h = lambda *s: torch.zeros(*s, dtype=torch.float16)
    src = torch.zeros(1, 3, 16, 16)
    for kw, msg in ((dict(src=torch.zeros(3, 16, 16)), "src must be"), (dict(src=src.double()), "src must be"),
                    (dict(src=torch.zeros(1, 1, 16, 16)), "3 channels"), (dict(src=torch.zeros(1, 16, 16, 4, dtype=torch.uint8)), "3 channels"),
                    (dict(out=h(255, 64)), "out must be"), (dict(out=h(256, 56)), "out must be"), (dict(out=torch.zeros(256, 64)), "out must be"),
                    (dict(out=h(256, 128)[:, ::2]), "out must be"), (dict(affine=torch.zeros(6)), "affine must be"), (dict(), "CUDA")):
        args = dict(src=src, out=h(256, 64))
        args.update(kw)
        with pytest.raises(ValueError, match="lpips_prep: .*" + msg):
            ops.lpips_prep(**args)
    with pytest.raises(ValueError, match="lpips_affine"):
        ops.lpips_affine("cpu", scale=(1.0, 0.0, 1.0))
    for x, msg in ((h(4, 12), "multiple of 8"), (h(4), "2-D"), (torch.zeros(4, 8), "x must be"), (h(4, 16)[:, :8], "CUDA"), (h(4, 8), "CUDA")):
        with pytest.raises(ValueError, match="relu_: .*" + msg):
            ops.relu_(x)
    x, lin = h(2 * 5 * 7, 64), torch.zeros(64)
    for kw, msg in ((dict(x=h(69, 64)), "x must be"), (dict(x=h(70, 520), lin_w=torch.zeros(520)), "multiple of 8 up to 512"),
                    (dict(x=h(70, 12), lin_w=torch.zeros(12)), "multiple of 8 up to 512"), (dict(lin_w=torch.zeros(32)), "lin_w must be"),
                    (dict(lin_w=lin.double()), "lin_w must be"), (dict(pairs=0), "pairs must be"), (dict(H=5.0), "H must be"),
                    (dict(pooled=h(2 * 2 * 3, 32)), "pooled must be"), (dict(pooled=h(11, 64)), "pooled must be"),
                    (dict(x=h(2 * 1 * 7, 64), H=1, pooled=h(8, 64)), "no 2x2 quad"), (dict(dmap=torch.zeros(1, 7, 5)), "dmap must be"),
                    (dict(out=torch.zeros(1)), "out must be"), (dict(), "CUDA")):
        args = dict(x=x, pairs=1, H=5, W=7, lin_w=lin)
        args.update(kw)
        with pytest.raises(ValueError, match="lpips_tap: .*" + msg):
            ops.lpips_tap(**args)
    with pytest.raises(ValueError, match="lpips_tap_workspace_bytes: "):
        ops.lpips_tap_workspace_bytes(1, 5, 7, 20)
    assert ops.lpips_tap_workspace_bytes(1, 37, 53, 64) == 17 * 8           # 19 x 27 quads, 32 per workgroup
    assert ops.lpips_tap_workspace_bytes(2, 5, 7, 512) == 2 * 3 * 8         # 3 x 4 quads, 4 per workgroup
    assert ops.LPIPS_CPAD == 64 and ops.LPIPS_MAX_C == 512


def test_invalid_arguments_are_rejected_without_a_gpu():
    h = lib.load()
    P = 4096
    Q = 1 << 20

    def prep(**k):
        a = dict(src=P, u8=0, N=1, H=16, W=16, affine=P, out=Q, ldo=64, dtype=0)
        a.update(k)
        return h.iir_lpips_prep(a["src"], a["u8"], a["N"], a["H"], a["W"], a["affine"], a["out"], a["ldo"], a["dtype"], None)
    for bad in (dict(src=None), dict(affine=None), dict(out=None), dict(N=0), dict(H=-1), dict(W=0), dict(H=32769), dict(ldo=56), dict(ldo=68),
                dict(out=Q + 8), dict(dtype=2), dict(out=P + 64), dict(src=P + 2), dict(affine=P + 4), dict(src=Q + 4096)):
        assert prep(**bad) == -1, bad
    relu = lambda x=P, ld=64, rows=4, C=64, dtype=0: h.iir_relu_f16(x, ld, rows, C, dtype, None)
    for bad in (dict(x=None), dict(x=P + 4), dict(rows=0), dict(C=0), dict(C=12), dict(ld=56), dict(ld=68, C=64), dict(dtype=3), dict(rows=1 << 40)):
        assert relu(**bad) == -1, bad

    def tap(**k):
        a = dict(x=P, ldx=64, pairs=1, H=5, W=7, C=64, lin=P, dtype=0, dmap=None, pooled=None, ldp=64, ws=1 << 20, ws_bytes=1 << 10, out=1 << 21)
        a.update(k)
        return h.iir_lpips_tap(a["x"], a["ldx"], a["pairs"], a["H"], a["W"], a["C"], a["lin"], a["dtype"], a["dmap"], a["pooled"], a["ldp"], a["ws"],
                               a["ws_bytes"], a["out"], None)
    for bad in (dict(x=None), dict(lin=None), dict(ws=None), dict(out=None), dict(pairs=0), dict(pairs=65536), dict(H=0), dict(W=40000), dict(C=0),
                dict(C=12), dict(C=520, ldx=520), dict(ldx=56), dict(ldx=68), dict(x=P + 8), dict(dtype=2), dict(ws=(1 << 20) + 4),
                dict(out=(1 << 21) + 4), dict(ws_bytes=4), dict(pooled=1 << 22, H=1), dict(pooled=1 << 22, ldp=56), dict(pooled=(1 << 22) + 8),
                dict(pooled=P + 64), dict(dmap=P + 128)):
        assert tap(**bad) == -1, bad
    need = h.iir_lpips_tap_workspace_bytes
    assert need(1, 5, 7, 64) == 8 and need(0, 5, 7, 64) == -1 and need(1, 5, 7, 12) == -1 and need(1, 5, 7, 520) == -1
    assert h.iir_abi_version() == 3


def test_header_declares_and_binds_the_entries():
    arity = {"iir_lpips_prep": 10, "iir_relu_f16": 6, "iir_lpips_tap_workspace_bytes": 4, "iir_lpips_tap": 15}
    assert set(arity) <= set(lib.declared_symbols())
    for fn, n in arity.items():
        restype, args = lib.SIGNATURES[fn]
        assert len(args) == n == len(lib.HEADER.functions[fn][1]), fn
        assert restype is (ctypes.c_int64 if fn.endswith("_bytes") else ctypes.c_int)
    text = open(lib.HEADER_PATH).read()
    assert text.count("losses/losses.py:81-95") >= 4 and "#define IIR_LPIPS_CPAD 64" in text and "#define IIR_ABI_VERSION 3" in text
    from instantir_amd import engine
    assert lib.MACROS["IIR_LPIPS_CPAD"] == engine.CPAD


# ---- the command line --------------------------------------------------------------------------------------------------------
def test_cli_flags(tmp_path):
    import instantir_amd.infer as cli
    parse = lambda *extra: cli.build_parser().parse_args(["--test_path", "x", "--synthetic", "tiny", *extra])
    weights = tmp_path / "lpips.pth"
    torch.save(LP.synthetic_state_dict(1, (8, 8, 8, 8, 8)), str(weights))
    assert cli.apply_pair_scorer("lpips", parse()) is None and cli.apply_pair_scorer("lpips", parse("--input_fidelity")) is None
    with pytest.raises(SystemExit, match="--lpips_path needs --gt_path or --input_fidelity"):
        cli.apply_pair_scorer("lpips", parse("--lpips_path", str(weights)))
    with pytest.raises(SystemExit, match="--lpips_path needs --gt_path or --input_fidelity"):      # and before any weight is built
        cli.main(parse("--lpips_path", str(weights)), "cpu")
    with pytest.raises(SystemExit, match="--lpips_lin_path needs --lpips_path"):
        cli.apply_pair_scorer("lpips", parse("--input_fidelity", "--lpips_lin_path", str(weights)))
    with pytest.raises(SystemExit, match="--lpips_path .*none.pth is not a file"):
        cli.apply_pair_scorer("lpips", parse("--input_fidelity", "--lpips_path", str(tmp_path / "none.pth")))
    with pytest.raises(SystemExit, match="--lpips_lin_path .*none.pth is not a file"):
        cli.apply_pair_scorer("lpips", parse("--input_fidelity", "--lpips_path", str(weights), "--lpips_lin_path", str(tmp_path / "none.pth")))
    args = parse("--gt_path", str(tmp_path), "--lpips_path", str(weights))
    assert cli.apply_pair_scorer("lpips", args) == {"path": str(weights), "lin_path": None}
    s = cli.apply_metrics(args)                                     # untouched by the flag: exactly its five keys
    assert s == {"gt_path": str(tmp_path), "input_fidelity": False, "metrics": ("psnr", "ssim"), "y_channel": False, "crop_border": 0}
    with pytest.raises(SystemExit):
        parse("--metrics", "lpips")
    torch.save({"net.slice1.0.weight": torch.zeros(8, 3, 3, 3)}, str(tmp_path / "broken.pth"))
    with pytest.raises(SystemExit, match="--lpips_path: LPIPS weights: missing key"):
        cli.build_pair_scorer("lpips", {"path": str(tmp_path / "broken.pth"), "lin_path": None}, "cpu")
