"""CPU: the DISTS contract (tests/dists_ref.py) against independent forms, its properties, the two weight formats, and every
refusal of instantir_amd.dists / the new ops / the new C entries / the new CLI flags that happens before a launch."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dists_ref as R
from instantir_amd import dists as DS
from instantir_amd import lib

NET_SHAPES = [(2, 3, 37, 53), (1, 3, 16, 19), (1, 3, 64, 48)]


def _pair(shape):
    g = torch.Generator().manual_seed(sum(shape))
    a = torch.rand(shape, generator=g)
    return a, (a + 0.1 * torch.randn(shape, generator=g)).clamp(0.0, 1.0)


def _small_net(seed=5, widths=(8, 16, 16, 24, 8)):
    convs, alpha, beta, mean, std = DS.parse_state_dict(DS.synthetic_state_dict(seed, widths))
    assert mean == R.MEAN and std == R.STD
    return convs, alpha, beta


# ---- the restatement against independent forms --------------------------------------------------------------------------------
def test_l2pool_equals_the_grouped_conv_form():
    """The DISTS package's own form: F.conv2d(x^2, hann, stride=2, padding=1, groups=C), then sqrt(. + 1e-12)."""
    g = torch.Generator().manual_seed(0)
    hann = torch.tensor(np.hanning(5)[1:-1], dtype=torch.float64)
    k = hann[:, None] * hann[None, :]
    k = k / k.sum()
    assert torch.equal(k, torch.tensor(R.HANN, dtype=torch.float64)[:, None] * torch.tensor(R.HANN, dtype=torch.float64)[None, :])
    for C, H, W in ((8, 5, 7), (8, 16, 16), (16, 37, 53), (8, 1, 1), (8, 2, 1)):
        x = torch.randn(2, C, H, W, generator=g, dtype=torch.float64).clamp_min(0.0)
        want = (F.conv2d(x * x, k[None, None].repeat(C, 1, 1, 1), stride=2, padding=1, groups=C) + 1e-12).sqrt()
        got = R.l2pool(x)
        assert tuple(got.shape) == (2, C, (H + 1) // 2, (W + 1) // 2)
        assert float((got - want).abs().max()) <= 4e-16 * float(want.max())
    assert float(R.l2pool(torch.zeros(1, 8, 3, 3))[0, 0, 0, 0]) == 1e-6


def test_raw_sum_variance_equals_two_pass_variance_on_the_network_shapes():
    """sigma^2 = E[a^2] - mu^2 from the raw sums (what the device path forms) against the two-pass form about the mean, on the
    three network shapes and the full-width net: every one of the twelve terms within 2e-16."""
    convs, alpha, beta, _, _ = DS.parse_state_dict(DS.synthetic_state_dict(21))
    for shape in NET_SHAPES:
        a, b = _pair(shape)
        s_raw, t_raw = R.dists(a, b, convs, alpha, beta)
        s_two, t_two = R.dists(a, b, convs, alpha, beta, two_pass=True)
        err = float((t_raw - t_two).abs().max())
        print(f"dists raw-sum vs two-pass {shape}: max term difference {err:.3e}; score {s_raw.tolist()}")
        assert err <= 2e-16 and float((s_raw - s_two).abs().max()) <= 2e-15


def test_constant_image_keeps_its_variance_below_the_bar():
    """The cancellation case of the raw-sum form: a constant 200 / 255 image has sigma^2 = 0; E[a^2] - mu^2 from fp64 sums of the
    fp32 pixel value stays below 1e-13 (the device test asks the same of the kernel's sums)."""
    v = (torch.tensor(200, dtype=torch.uint8).float() / 255.0)
    for H, W in ((16, 16), (17, 23), (512, 512)):
        x = v.expand(1, 3, H, W).contiguous()
        s, _ = R.sums(x, x)
        s = np.asarray(s, dtype=np.float64)
        n = H * W
        var = s[..., 2] / n - (s[..., 0] / n) ** 2
        assert float(np.abs(var).max()) < 1e-13
        s1, s2 = R.similarities(s, n)
        assert float((s1 - 1).abs().max()) <= 1e-15 and float((s2 - 1).abs().max()) <= 1e-6


def test_model_identities():
    convs, alpha, beta = _small_net()
    a, b = _pair((2, 3, 19, 16))
    sab, tab = R.dists(a, b, convs, alpha, beta)
    sba, tba = R.dists(b, a, convs, alpha, beta)
    saa, taa = R.dists(a, a, convs, alpha, beta)
    assert float(saa.abs().max()) <= 1e-12                                   # DISTS(a, a) = 0
    assert float((sab - sba).abs().max()) <= 1e-15 and float((tab - tba).abs().max()) <= 1e-15       # symmetry
    assert tuple(tab.shape) == (2, 6, 2) and float((1.0 - tab.sum(dim=(1, 2)) - sab).abs().max()) <= 1e-15
    assert bool((sab > 0).all()) and bool((sab < 1).all())
    for st in (torch.float16, torch.bfloat16):
        for acc in (torch.float32, torch.float64):
            ss, ts = R.dists(a, b, convs, alpha, beta, storage=st, accumulate=acc)
            assert torch.equal(ts[:, 0], tab[:, 0])                          # stage 0 never sees a 16-bit type
            assert 0 < float((ss - sab).abs().max()) < 0.05


# ---- the weight formats ---------------------------------------------------------------------------------------------------------
def _two_formats(tmp_path, widths=(8, 16, 16, 24, 8), norm=False):
    whole = DS.synthetic_state_dict(9, widths)
    tv = {"features." + k.split(".", 1)[1]: v for k, v in whole.items() if k.startswith("stage")}
    tv["classifier.0.weight"] = torch.zeros(4, 4)                         # what a torchvision file also holds
    wt = {"alpha": whole["alpha"], "beta": whole["beta"]}
    whole["stage2.4.filter"] = torch.zeros(8, 1, 3, 3)                    # the L2 pools' buffers of a whole DISTS state dict
    if norm:
        whole["mean"] = torch.tensor(R.MEAN).view(1, 3, 1, 1)
        whole["std"] = torch.tensor(R.STD).view(1, 3, 1, 1)
    paths = [str(tmp_path / n) for n in ("vgg16.pth", "weights.pt", "dists_whole.pth")]
    for p, sd in zip(paths, (tv, wt, whole)):
        torch.save(sd, p)
    return paths, whole


def test_both_formats_load_to_equal_tensors(tmp_path):
    (tv, wt, whole), sd = _two_formats(tmp_path)
    ca, aa, ba, ma, sa = DS.load_weights(tv, wt)
    cb, ab, bb, mb, sb = DS.load_weights(whole)
    assert len(ca) == len(cb) == 13 and all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(ca, cb))
    assert torch.equal(aa, ab) and torch.equal(ba, bb) and aa.dtype == torch.float64 and tuple(aa.shape) == (3 + 8 + 16 + 16 + 24 + 8,)
    assert torch.equal(aa, sd["alpha"].double().reshape(-1)) and not torch.equal(aa, ba)
    assert [w.shape[0] for w, _ in ca] == [8, 8, 16, 16, 16, 16, 16, 24, 24, 24, 8, 8, 8]
    assert ma == mb == R.MEAN and sa == sb == R.STD                       # a file without mean / std gets the ImageNet constants
    (_, _, whole2), _ = _two_formats(tmp_path, norm=True)
    _, _, _, m2, s2 = DS.load_weights(whole2)
    assert np.allclose(m2, R.MEAN, rtol=1e-7) and np.allclose(s2, R.STD, rtol=1e-7)
    m = DS.DISTS.from_files(whole, device="cpu")
    assert m.widths == (3, 8, 16, 16, 24, 8) and m.padded == (3, 64, 64, 64, 64, 64) and m.offsets[-1] == 3 + 5 * 64
    assert tuple(m.w[0][0].shape) == (64, 3, 3, 64) and m.w[0][0].dtype == torch.float16 and float(m.w[0][0][8:].abs().max()) == 0.0
    # the weighting reads the real channels of every stage, in the order of alpha / beta, and the weights sum to 1
    total = float(aa.sum() + ba.sum())
    assert abs(float(m.alpha.sum() + m.beta.sum()) - 1.0) <= 1e-15
    assert m.index[0, :3].tolist() == [0, 1, 2] and m.index[2, :16].tolist() == list(range(67, 83)) and m.index[5, :8].tolist() == list(range(259, 267))
    assert torch.equal(m.alpha[2, :16] * total, aa[11:27]) or float((m.alpha[2, :16] * total - aa[11:27]).abs().max()) <= 1e-15
    assert float(m.alpha[0, 3:].abs().max()) == 0.0 and float(m.beta[5, 8:].abs().max()) == 0.0


def test_loader_refusals_name_the_key(tmp_path):
    sd = DS.synthetic_state_dict(9, (8, 8, 8, 8, 8))
    bad = dict(sd)
    del bad["stage3.12.bias"]
    with pytest.raises(ValueError, match=r"DISTS weights: missing key stage3\.12\.bias"):
        DS.parse_state_dict(bad)
    for key in ("alpha", "beta"):
        bad = dict(sd)
        del bad[key]
        with pytest.raises(ValueError, match=f"missing key {key}"):
            DS.parse_state_dict(bad)
        bad[key] = torch.zeros(1, 1475, 1, 1)
        with pytest.raises(ValueError, match=rf"{key} must be shaped \(1, 43, 1, 1\)"):
            DS.parse_state_dict(bad)
    bad = dict(sd)
    bad["stage2.7.weight"] = torch.zeros(8, 8, 5, 5)
    with pytest.raises(ValueError, match=r"stage2\.7\.weight must be a \(Cout, Cin, 3, 3\) kernel"):
        DS.parse_state_dict(bad)
    bad = dict(sd)
    bad["stage1.0.weight"], bad["stage1.0.bias"] = torch.zeros(12, 3, 3, 3), torch.zeros(12)
    with pytest.raises(ValueError, match=r"stage1\.0\.weight has 12 output channels"):
        DS.parse_state_dict(bad)
    bad = dict(sd)
    bad["stage4.17.weight"] = torch.zeros(8, 16, 3, 3)
    with pytest.raises(ValueError, match=r"stage4\.17\.weight reads 16 channels but the layer before it writes 8"):
        DS.parse_state_dict(bad)
    bad = dict(sd)
    bad["mean"], bad["std"] = torch.zeros(4), torch.ones(3)
    with pytest.raises(ValueError, match="mean must hold 3 values"):
        DS.parse_state_dict(bad)
    tv = {"features." + k.split(".", 1)[1]: v for k, v in sd.items() if k.startswith("stage")}
    with pytest.raises(ValueError, match="needs alpha and beta too"):
        DS.parse_state_dict(tv)
    with pytest.raises(ValueError, match=r"missing key features\.28\.weight"):
        DS.parse_state_dict({k: v for k, v in tv.items() if k != "features.28.weight"}, {"alpha": sd["alpha"], "beta": sd["beta"]})
    with pytest.raises(ValueError, match="missing key beta"):
        DS.parse_state_dict(tv, {"alpha": sd["alpha"]})
    with pytest.raises(ValueError, match="DISTS.synthetic: widths must be five positive multiples of 8"):
        DS.synthetic_state_dict(1, (8, 8, 8, 12, 8))
    a = DS.synthetic_state_dict(4)
    assert tuple(a["alpha"].shape) == (1, 1475, 1, 1) and 0 <= float(a["beta"].min()) and float(a["alpha"].max()) < 1


# ---- refusals before any launch -----------------------------------------------------------------------------------------------
def test_module_refusals():
    m = DS.DISTS.synthetic(3, (8, 8, 8, 8, 8), device="cpu")
    ok = torch.zeros(1, 3, 16, 16)
    with pytest.raises(ValueError, match="DISTS: the smallest side is 16"):
        m(torch.zeros(1, 3, 15, 40), torch.zeros(1, 3, 15, 40))
    with pytest.raises(ValueError, match="but its counterpart"):
        m(ok, torch.zeros(1, 3, 16, 17))
    with pytest.raises(ValueError, match="3 channels"):
        m(torch.zeros(1, 1, 16, 16), torch.zeros(1, 1, 16, 16))
    with pytest.raises(ValueError, match="a: expected"):
        m("a.png", ok)
    with pytest.raises(ValueError, match="no host path"):
        m(ok, ok)
    with pytest.raises(ValueError, match="dtype must be"):
        DS.DISTS.synthetic(3, (8, 8, 8, 8, 8), device="cpu", dtype=torch.float32)
    full = DS.DISTS.synthetic(3, (64, 8, 8, 8, 8), device="cpu")
    full._check_geometry(2048, 2048)
    assert full._largest_activation_bytes(2048, 2048) == 1 << 30
    with pytest.raises(ValueError, match=r"DISTS of a 4096x2048 pair: its largest activation \(2147483648 bytes\) reaches 2 GiB"):
        full._check_geometry(4096, 2048)
    assert full.stage_sizes(37, 53) == [(37, 53), (37, 53), (19, 27), (10, 14), (5, 7), (3, 4)]
    from instantir_amd import metrics as M
    with pytest.raises(ValueError, match="smallest side"):
        M.dists(torch.zeros(3, 8, 8), torch.zeros(3, 8, 8), m)
    with pytest.raises(ValueError, match="the DISTS model lives on cpu"):
        M.dists(ok, ok, m, device="cuda:0")
    assert M.METRICS == ("psnr", "ssim")


def test_evaluate_keys_are_unchanged_without_a_model(monkeypatch):
    """`evaluate` gains "dists" / "dists_mean" only when a model is given (the PSNR / SSIM launch is stood in for: no GPU here)."""
    import inspect
    from instantir_amd import metrics as M
    for fn in (M.evaluate, M.input_fidelity):
        p = inspect.signature(fn).parameters
        assert p["dists_model"].default is None and p["lpips_model"].default is None and list(p)[-1] == "dists_model"
    monkeypatch.setattr(M, "_run", lambda *a, **k: ({"psnr": [30.0], "ssim": [0.5]}, True))

    class Fake:
        device = torch.device("cpu")

        def __call__(self, a, b):
            return torch.tensor([0.25], dtype=torch.float64)
    x = torch.zeros(1, 3, 16, 16)
    assert M.evaluate(x, x) == {"psnr": [30.0], "ssim": [0.5], "psnr_mean": 30.0, "ssim_mean": 0.5}
    with_model = M.evaluate(x, x, dists_model=Fake())
    assert set(with_model) == {"psnr", "ssim", "dists", "psnr_mean", "ssim_mean", "dists_mean"} and with_model["dists"] == [0.25]
    assert set(M.evaluate(x, x, lpips_model=Fake(), dists_model=Fake())) == set(with_model) | {"lpips", "lpips_mean"}
    assert M.dists(x[0], x[0], Fake()) == 0.25 and M.dists(x, x, Fake()) == [0.25]


def test_ops_wrapper_refusals():
    from instantir_amd import ops
    h = lambda *s: torch.zeros(*s, dtype=torch.float16)
    x = h(2 * 5 * 7, 64)
    for kw, msg in ((dict(x=h(69, 64)), "x must be"), (dict(x=h(70, 520)), "multiple of 8 up to 512"), (dict(x=h(70, 12)), "multiple of 8 up to 512"),
                    (dict(x=h(70)), "2-D"), (dict(images=0), "images must be"), (dict(H=5.0), "H must be"), (dict(out=h(23, 64)), "out must be"),
                    (dict(out=h(24, 56)), "out must be"), (dict(out=torch.zeros(24, 64, dtype=torch.bfloat16)), "x's dtype"),
                    (dict(out=h(24, 128)[:, ::2]), "out must be"), (dict(), "CUDA")):
        args = dict(x=x, images=2, H=5, W=7)
        args.update(kw)
        with pytest.raises(ValueError, match="dists_l2pool: .*" + msg):
            ops.dists_l2pool(**args)
    for kw, msg in ((dict(x=h(69, 64)), "x must be"), (dict(x=h(70, 520)), "multiple of 8 up to 512"), (dict(pairs=0), "pairs must be"),
                    (dict(W=-1), "W must be"), (dict(out=torch.zeros(1, 64, 4, dtype=torch.float64)), "out must be"),
                    (dict(out=torch.zeros(1, 64, 5)), "out must be"), (dict(), "CUDA")):
        args = dict(x=x, pairs=1, H=5, W=7)
        args.update(kw)
        with pytest.raises(ValueError, match="dists_stats: .*" + msg):
            ops.dists_stats(**args)
    a = torch.zeros(1, 3, 16, 16)
    for kw, msg in ((dict(a=torch.zeros(3, 16, 16)), "a must be"), (dict(b=a.double()), "b must be"), (dict(b=torch.zeros(1, 3, 16, 17)), "share a dtype and a shape"),
                    (dict(b=torch.zeros(1, 16, 16, 3, dtype=torch.uint8)), "share a dtype and a shape"),
                    (dict(a=torch.zeros(1, 1, 16, 16), b=torch.zeros(1, 1, 16, 16)), "3 channels"),
                    (dict(out=torch.zeros(1, 3, 5)), "out must be"), (dict(), "CUDA")):
        args = dict(a=a, b=a.clone())
        args.update(kw)
        with pytest.raises(ValueError, match="dists_image_stats: .*" + msg):
            ops.dists_image_stats(**args)
    with pytest.raises(ValueError, match="dists_stats_workspace_bytes: "):
        ops.dists_stats_workspace_bytes(1, 5, 7, 20)
    # the share of a workgroup follows from H * W and C alone: NT / (C / 8) pixels at once, 8 .. 64 of them per lane
    assert ops.dists_stats_workspace_bytes(1, 37, 53, 64) == 8 * 64 * 5 * 8             # 1961 pixels, 32 x 8 per workgroup
    assert ops.dists_stats_workspace_bytes(2, 5, 7, 512) == 2 * 2 * 512 * 5 * 8         # 35 pixels, 4 x 8 per workgroup
    assert ops.dists_stats_workspace_bytes(1, 1024, 1024, 64) == 1024 * 64 * 5 * 8      # 32 x 32 per workgroup
    assert ops.dists_image_stats_workspace_bytes(2, 17, 23) == 2 * 1 * 3 * 5 * 8
    assert ops.DISTS_STATS == 5
    aff = ops.dists_affine("cpu")
    assert aff.dtype == torch.float64 and aff.tolist() == [2 * m - 1 for m in R.MEAN] + [2 * s for s in R.STD]


def test_invalid_arguments_are_rejected_without_a_gpu():
    """IIR_EINVAL before any HIP call; every call below is invalid, so none of them launches."""
    h = lib.load()
    P, Q, WS, OUT = 4096, 1 << 20, 1 << 22, 1 << 23

    def pool(**k):
        a = dict(x=P, ldx=64, images=2, H=5, W=7, C=64, dtype=0, out=Q, ldo=64)
        a.update(k)
        return h.iir_dists_l2pool(a["x"], a["ldx"], a["images"], a["H"], a["W"], a["C"], a["dtype"], a["out"], a["ldo"], None)
    for bad in (dict(x=None), dict(out=None), dict(x=P + 8), dict(out=Q + 8), dict(images=0), dict(H=0), dict(W=-3), dict(H=32769), dict(C=0),
                dict(C=12), dict(C=520, ldx=520, ldo=520), dict(ldx=56), dict(ldx=68), dict(ldo=56), dict(ldo=68), dict(dtype=2),
                dict(out=P + 64), dict(out=P - 64), dict(images=1 << 30, H=32768, W=32768, C=512, ldx=512, ldo=512)):
        assert pool(**bad) == -1, bad

    def stats(**k):
        a = dict(x=P, ldx=64, pairs=1, H=5, W=7, C=64, dtype=0, ws=WS, ws_bytes=1 << 20, out=OUT)
        a.update(k)
        return h.iir_dists_stats(a["x"], a["ldx"], a["pairs"], a["H"], a["W"], a["C"], a["dtype"], a["ws"], a["ws_bytes"], a["out"], None)
    for bad in (dict(x=None), dict(ws=None), dict(out=None), dict(pairs=0), dict(pairs=65536), dict(H=0), dict(W=40000), dict(C=0), dict(C=12),
                dict(C=520, ldx=520), dict(ldx=56), dict(ldx=68), dict(x=P + 8), dict(dtype=2), dict(ws=WS + 4), dict(out=OUT + 4),
                dict(ws_bytes=64 * 5 * 8 - 8)):
        assert stats(**bad) == -1, bad

    def image(**k):
        a = dict(a=P, b=Q, u8=0, N=1, H=16, W=16, ws=WS, ws_bytes=1 << 20, out=OUT)
        a.update(k)
        return h.iir_dists_image_stats(a["a"], a["b"], a["u8"], a["N"], a["H"], a["W"], a["ws"], a["ws_bytes"], a["out"], None)
    for bad in (dict(a=None), dict(b=None), dict(ws=None), dict(out=None), dict(N=0), dict(N=65536), dict(H=0), dict(W=32769), dict(a=P + 2),
                dict(b=Q + 1), dict(ws=WS + 4), dict(out=OUT + 4), dict(ws_bytes=3 * 5 * 8 - 8)):
        assert image(**bad) == -1, bad
    need = h.iir_dists_stats_workspace_bytes
    assert need(1, 5, 7, 64) == 64 * 5 * 8 and need(0, 5, 7, 64) == -1 and need(1, 5, 7, 12) == -1 and need(1, 5, 7, 520) == -1
    assert h.iir_dists_image_stats_workspace_bytes(1, 16, 16) == 3 * 5 * 8 and h.iir_dists_image_stats_workspace_bytes(1, 0, 16) == -1
    assert h.iir_abi_version() == 3


def test_header_declares_and_binds_the_entries():
    arity = {"iir_dists_l2pool": 10, "iir_dists_stats_workspace_bytes": 4, "iir_dists_stats": 11, "iir_dists_image_stats_workspace_bytes": 3,
             "iir_dists_image_stats": 10}
    assert set(arity) <= set(lib.declared_symbols())
    for fn, n in arity.items():
        restype, args = lib.SIGNATURES[fn]
        assert len(args) == n == len(lib.HEADER.functions[fn][1]), fn
        assert restype is (ctypes.c_int64 if fn.endswith("_bytes") else ctypes.c_int)
    text = open(lib.HEADER_PATH).read()
    assert "#define IIR_DISTS_STATS 5" in text and "#define IIR_ABI_VERSION 3" in text and 'section 7 "DISTS"' in text
    assert len(lib.HEADER.structs) == 8                                   # the entries take plain arguments: no new struct


# ---- the command line -----------------------------------------------------------------------------------------------------------
def test_cli_flags(tmp_path):
    import instantir_amd.infer as cli
    parse = lambda *extra: cli.build_parser().parse_args(["--test_path", "x", "--synthetic", "tiny", *extra])
    weights = tmp_path / "dists.pth"
    torch.save(DS.synthetic_state_dict(1, (8, 8, 8, 8, 8)), str(weights))
    assert cli.apply_pair_scorer("dists", parse()) is None and cli.apply_pair_scorer("dists", parse("--input_fidelity")) is None
    with pytest.raises(SystemExit, match="--dists_path needs --gt_path or --input_fidelity"):
        cli.apply_pair_scorer("dists", parse("--dists_path", str(weights)))
    with pytest.raises(SystemExit, match="--dists_path needs --gt_path or --input_fidelity"):      # and before any weight is built
        cli.main(parse("--dists_path", str(weights)), "cpu")
    with pytest.raises(SystemExit, match="--dists_weights_path needs --dists_path"):
        cli.apply_pair_scorer("dists", parse("--input_fidelity", "--dists_weights_path", str(weights)))
    with pytest.raises(SystemExit, match="--dists_path .*none.pth is not a file"):
        cli.apply_pair_scorer("dists", parse("--input_fidelity", "--dists_path", str(tmp_path / "none.pth")))
    with pytest.raises(SystemExit, match="--dists_weights_path .*none.pth is not a file"):
        cli.apply_pair_scorer("dists", parse("--input_fidelity", "--dists_path", str(weights), "--dists_weights_path", str(tmp_path / "none.pth")))
    args = parse("--gt_path", str(tmp_path), "--dists_path", str(weights))
    assert cli.apply_pair_scorer("dists", args) == {"path": str(weights), "weights_path": None}
    assert cli.apply_pair_scorer("lpips", args) is None
    s = cli.apply_metrics(args)                                     # untouched by the flag: exactly its five keys
    assert s == {"gt_path": str(tmp_path), "input_fidelity": False, "metrics": ("psnr", "ssim"), "y_channel": False, "crop_border": 0}
    with pytest.raises(SystemExit):
        parse("--metrics", "dists")
    torch.save({"stage1.0.weight": torch.zeros(8, 3, 3, 3)}, str(tmp_path / "broken.pth"))
    with pytest.raises(SystemExit, match="--dists_path: DISTS weights: missing key"):
        cli.build_pair_scorer("dists", {"path": str(tmp_path / "broken.pth"), "weights_path": None}, "cpu")
