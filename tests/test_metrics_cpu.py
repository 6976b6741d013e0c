"""CPU: the image-metrics contract (DESIGN.md section 7 "Image metrics") without a GPU -- the fp64 restatement of
tests/metrics_ref.py against scipy's 2-D correlation and against closed forms, the fp32 restatement inside the derived bound,
every refusal of `ops.image_metrics`, `instantir_amd.metrics` and the CLI flags, and the C entry's argument checks and ABI."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import metrics_ref as R
from instantir_amd import lib


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def test_windowed_moments_equal_scipys_valid_correlation():
    from scipy.signal import correlate2d
    a, b = (R.prepare(x) for x in R.pair(3, (1, 3, 29, 37), True, True))
    win = R.window64()
    assert abs(win.sum() - 1.0) < 1e-15 and win.shape == (11, 11)
    got = R.moments(a, b)
    for m, src in zip(got, (a, b, a * a, b * b, a * b)):
        assert m.shape == (1, 3, 19, 27)
        for c in range(3):
            want = correlate2d(src[0, c], win, mode="valid")
            assert np.abs(m[0, c] - want).max() <= 1e-12 * np.abs(want).max()


def test_closed_forms():
    a8, b8 = R.pair(4, (2, 3, 24, 31), True, True)
    same = R.evaluate(a8, a8)
    assert np.array_equal(same[:, 0], [0.0, 0.0]) and np.abs(same[:, 1] - 1.0).max() < 1e-12
    assert R.psnr_from_mse(same[0, 0]) == float("inf")
    ab, ba = R.evaluate(a8, b8), R.evaluate(b8, a8)
    assert np.array_equal(ab[:, 0], ba[:, 0]) and np.abs(ab[:, 1] - ba[:, 1]).max() < 1e-14
    assert 0.0 < ab[0, 1] < 1.0 and ab[0, 0] > 0
    # a constant offset d: PSNR = 20 log10(255 / d)
    base = np.random.default_rng(0).integers(0, 200, (1, 20, 20, 3), dtype=np.uint8)
    for d in (1, 7, 50):
        m = R.evaluate(base, base + np.uint8(d))[0, 0]
        assert m == d * d and abs(R.psnr_from_mse(m) - 20 * math.log10(255 / d)) < 1e-12
    # two constant images: the structure term is 1, the luminance term is what remains
    for m1, m2 in ((10, 200), (0, 255), (128, 128)):
        x = np.full((1, 15, 17, 1), m1, np.uint8), np.full((1, 15, 17, 1), m2, np.uint8)
        want = (2 * m1 * m2 + R.C1) / (m1 * m1 + m2 * m2 + R.C1)
        assert abs(R.evaluate(*x)[0, 1] - want) < 1e-12


def test_luma_of_white_black_and_the_primaries():
    px = lambda r, g, b: R.luma(np.array([r, g, b], np.float64).reshape(1, 3, 1, 1))[0, 0, 0, 0]
    assert abs(px(255, 255, 255) - 235.0) < 1e-12 and px(0, 0, 0) == 16.0
    assert abs(px(255, 0, 0) - (16 + 65.481)) < 1e-12 and abs(px(0, 255, 0) - (16 + 128.553)) < 1e-12
    assert abs(px(0, 0, 255) - (16 + 24.966)) < 1e-12
    a8, b8 = R.pair(5, (1, 3, 20, 22), True, True)
    y = R.evaluate(a8, b8, y_channel=True)
    assert y.shape == (1, 2) and not np.array_equal(y, R.evaluate(a8, b8))


def test_crop_border_equals_slicing_first():
    a8, b8 = R.pair(6, (2, 3, 30, 33), True, True)
    af, bf = R.pair(6, (2, 3, 30, 33), False, False)
    for c in (1, 4, 9):
        assert np.array_equal(R.evaluate(a8, b8, crop_border=c), R.evaluate(a8[:, c:-c, c:-c], b8[:, c:-c, c:-c]))
        sl = lambda x: np.ascontiguousarray(x[:, :, c:-c, c:-c])
        assert np.array_equal(R.evaluate(af, bf, crop_border=c, y_channel=True), R.evaluate(sl(af), sl(bf), y_channel=True))
    with pytest.raises(ValueError):
        R.evaluate(a8, b8, crop_border=15)
    assert np.isnan(R.evaluate(a8, b8, crop_border=10)[:, 1]).all()          # 10 x 13 remain: an MSE, no window


def test_quantize_is_the_rounding_of_a_saved_image():
    x = np.array([0.0, 0.5 / 255, 0.49 / 255, 1.0, 1.2, -0.3, 127.5 / 255], np.float32).reshape(1, 1, 1, 7)
    assert R.to255(x, True).ravel().tolist() == [0, 1, 0, 255, 255, 0, 128]
    assert np.array_equal(R.to255(x, False), x.astype(np.float64) * 255.0)
    a8, _ = R.pair(7, (1, 3, 12, 12), True, True)
    as_f = (a8.transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255.0))
    assert np.array_equal(R.to255(as_f, True), R.to255(a8))                      # an 8-bit image survives the trip through [0, 1]


@pytest.mark.parametrize("form", sorted(R.SOURCE_FORMS))
@pytest.mark.parametrize("si", range(len(R.GPU_SHAPES)))
def test_fp32_restatement_is_inside_the_bound(si, form):
    """The rehearsal of the GPU test: the arithmetic the kernel performs, restated on the host, against the fp64 contract."""
    shape, c = R.GPU_SHAPES[si]
    a_u8, b_u8, q = R.SOURCE_FORMS[form]
    a, b = R.pair(11 + si, shape, a_u8, b_u8)
    for y in ((False, True) if shape[1] == 3 else (False,)):
        want = R.evaluate(a, b, c, y, q)
        got = R.evaluate32(a, b, c, y, q)
        b_mse, b_ssim = R.bounds(a_u8 or q[0], b_u8 or q[1], y)
        if form in ("u8_u8", "f32q_u8") and not y:
            assert np.array_equal(got[:, 0], want[:, 0])
        assert np.abs(got[:, 0] - want[:, 0]).max() <= b_mse and np.abs(got[:, 1] - want[:, 1]).max() <= b_ssim
        only = R.evaluate32(a, b, c, y, q, what=("psnr",))
        assert np.isnan(only[:, 1]).all() and np.abs(only[:, 0] - want[:, 0]).max() <= b_mse
    assert 1e-4 < R.bounds(True, True, False)[1] < 1e-2 and R.bounds(False, False, True)[0] < 0.2


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_ops_wrapper_refusals():
    from instantir_amd import ops
    f = lambda *s: torch.zeros(*s)
    u = lambda *s: torch.zeros(*s, dtype=torch.uint8)
    ok = f(1, 3, 16, 16)
    for kw, msg in ((dict(a=f(3, 16, 16)), "a must be"), (dict(b=f(1, 3, 16, 16).double()), "b must be"),
                    (dict(a=f(1, 3, 16, 32)[:, :, :, ::2]), "a must be"), (dict(b="x"), "b must be"),
                    (dict(b=f(1, 3, 16, 17)), "b is"), (dict(b=u(1, 16, 16, 1)), "b is"), (dict(a=f(1, 2, 16, 16), b=f(1, 2, 16, 16)), "1 or 3 channels"),
                    (dict(a=f(1, 1, 16, 16), b=u(1, 16, 16, 1), y_channel=True), "y_channel"),
                    (dict(crop_border=-1), "crop_border"), (dict(crop_border=1.5), "crop_border"), (dict(crop_border=True), "crop_border"),
                    (dict(crop_border=3), "leaves less than 11"), (dict(crop_border=8, what="psnr"), "leaves less than 1"),
                    (dict(a=f(1, 3, 10, 40), b=f(1, 3, 10, 40)), "leaves less than 11"),
                    (dict(what=()), "what"), (dict(what="mse"), "what"), (dict(what=("psnr", "lpips")), "what"),
                    (dict(quantize=True), "quantize"), (dict(quantize=(True,)), "quantize"),
                    (dict(), "CUDA")):
        args = dict(a=ok, b=ok)
        args.update(kw)
        with pytest.raises(ValueError, match="image_metrics: .*" + msg):
            ops.image_metrics(**args)


def test_metrics_module_refusals():
    from PIL import Image
    from instantir_amd import metrics as M
    im = Image.new("RGB", (20, 16))
    arr = np.zeros((16, 20, 3), np.uint8)
    for fn in (M.psnr, M.ssim, M.evaluate):
        with pytest.raises(ValueError, match="a: expected"):
            fn("a.png", im)
        with pytest.raises(ValueError, match="b: a list must hold PIL images"):
            fn(im, [])
        with pytest.raises(ValueError, match="b: the images of a list must share a size"):
            fn([im, im], [im, Image.new("RGB", (21, 16))])
        with pytest.raises(ValueError, match="a: expected uint8 or floating-point"):
            fn(arr.astype(np.int32), im)
        with pytest.raises(ValueError, match="b: expected an image or a batch"):
            fn(arr, np.zeros((1, 1, 16, 20, 3), np.uint8))
        with pytest.raises(ValueError, match="b is .* but its counterpart"):
            fn(im, Image.new("RGB", (20, 17)))
        with pytest.raises(ValueError, match="crop_border"):
            fn(im, arr, crop_border=-2)
        with pytest.raises(ValueError, match="y_channel needs 3 channels"):
            fn(Image.new("L", (20, 16)), arr[:, :, 0], y_channel=True)
        with pytest.raises(ValueError, match="quantize"):
            fn(im, arr, quantize=(True, False, True))
        with pytest.raises(ValueError, match="1 or 3 channels"):
            fn(np.zeros((16, 20, 2), np.uint8), np.zeros((16, 20, 2), np.uint8))
    with pytest.raises(ValueError, match="crop_border 3 leaves less than 11"):
        M.ssim(im, arr, crop_border=3)
    with pytest.raises(ValueError, match="crop_border 8 leaves less than 1 "):
        M.psnr(im, arr, crop_border=8)
    with pytest.raises(ValueError, match="metrics must name"):
        M.evaluate(im, arr, metrics=("psnr", "fid"))
    with pytest.raises(ValueError, match="filter must be one of"):
        M.input_fidelity(im, arr, filter="nearest")
    with pytest.raises(ValueError, match="restored holds"):
        M.input_fidelity(im, Image.new("L", (10, 8)))
    with pytest.raises(ValueError, match="restored: expected"):
        M.input_fidelity(None, im)
    assert M.psnr_from_mse(0.0) == math.inf and abs(M.psnr_from_mse(1.0) - 20 * math.log10(255)) < 1e-12


def test_host_forms_become_the_kernels_two_layouts():
    from PIL import Image
    from instantir_amd import images as M
    arr = np.random.default_rng(1).integers(0, 255, (16, 20, 3), dtype=np.uint8)
    forms = [Image.fromarray(arr), [Image.fromarray(arr)], arr, arr[None], torch.from_numpy(arr), torch.from_numpy(arr[None])]
    for i, x in enumerate(forms):
        t, single = M.host_source(x, "a")
        assert t.dtype == torch.uint8 and tuple(t.shape) == (1, 16, 20, 3) and np.array_equal(t[0].numpy(), arr)
        assert single == (i in (0, 2, 4))
    as_f = arr.astype(np.float32) / 255
    for x in (as_f, as_f[None], torch.from_numpy(as_f).permute(2, 0, 1), torch.from_numpy(as_f).permute(2, 0, 1)[None].double()):
        t, _ = M.host_source(x, "a")
        assert t.dtype == torch.float32 and tuple(t.shape) == (1, 3, 16, 20)
        assert np.array_equal(t[0].permute(1, 2, 0).numpy(), as_f)
    g, _ = M.host_source(Image.fromarray(arr[:, :, 0]), "a")
    assert tuple(g.shape) == (1, 16, 20, 1)
    rgba, _ = M.host_source(Image.fromarray(arr).convert("RGBA"), "a")
    assert tuple(rgba.shape) == (1, 16, 20, 3)


def test_cli_flag_refusals(tmp_path):
    from PIL import Image
    import instantir_amd.infer as cli
    parse = lambda *extra: cli.build_parser().parse_args(["--test_path", "x", "--synthetic", "tiny", *extra])
    assert cli.apply_metrics(parse()) is None
    for extra, flag in ((["--metrics", "psnr"], "--metrics "), (["--metrics_y"], "--metrics_y"), (["--metrics_crop", "2"], "--metrics_crop")):
        with pytest.raises(SystemExit, match=flag + ".*needs --gt_path or --input_fidelity"):
            cli.apply_metrics(parse(*extra))
        with pytest.raises(SystemExit, match="needs --gt_path or --input_fidelity"):       # and before any weight is built
            cli.main(parse(*extra), "cpu")
    with pytest.raises(SystemExit, match="--metrics_crop must be >= 0"):
        cli.apply_metrics(parse("--input_fidelity", "--metrics_crop", "-1"))
    with pytest.raises(SystemExit, match="is not a directory"):
        cli.apply_metrics(parse("--gt_path", str(tmp_path / "none")))
    with pytest.raises(SystemExit):
        parse("--metrics", "lpips")
    s = cli.apply_metrics(parse("--gt_path", str(tmp_path), "--metrics", "ssim", "--metrics_y", "--metrics_crop", "4"))
    assert s == {"gt_path": str(tmp_path), "input_fidelity": False, "metrics": ("ssim",), "y_channel": True, "crop_border": 4}
    s = cli.apply_metrics(parse("--input_fidelity"))
    assert s["metrics"] == ("psnr", "ssim") and s["gt_path"] is None and s["input_fidelity"] and s["crop_border"] == 0
    # the ground truth of an input: same name, output size
    s = cli.apply_metrics(parse("--gt_path", str(tmp_path)))
    Image.new("RGB", (24, 16)).save(tmp_path / "a.png")
    assert cli.gt_image(s, "a.png", (24, 16)).size == (24, 16)
    with pytest.raises(SystemExit, match="b.png does not exist"):
        cli.gt_image(s, "b.png", (24, 16))
    with pytest.raises(SystemExit, match="a.png is 24x16 but the output is 16x24"):
        cli.gt_image(s, "a.png", (16, 24))
    # the report
    line = cli.write_metrics(s, {"a.png": {"psnr": 30.0, "ssim": 0.5}, "b.png": {"psnr": 20.0, "ssim": 1.0}}, str(tmp_path), 1, 2)
    import json
    rep = json.load(open(tmp_path / "metrics.rank1.json"))
    assert rep["mean"] == {"psnr": 25.0, "ssim": 0.75} and rep["files"]["b.png"]["psnr"] == 20.0 and rep["settings"]["metrics"] == ["psnr", "ssim"]
    assert "2 file(s)" in line and "psnr 25.0000" in line
    cli.write_metrics(s, {}, str(tmp_path))
    assert json.load(open(tmp_path / "metrics.json"))["files"] == {}


# ---- the C entry ---------------------------------------------------------------------------------------------------------------
def _desc(**kw):
    d = lib.MetricsDesc()
    d.a = d.b = d.ws = d.out = 4096
    d.N, d.C, d.H, d.W = 1, 3, 32, 40
    d.what = lib.METRIC_PSNR | lib.METRIC_SSIM
    d.ws_bytes = 1 << 20
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_abi_is_additive():
    assert sorted(lib.declared_symbols()) == sorted(lib.SIGNATURES)
    assert {"iir_image_metrics", "iir_image_metrics_workspace_bytes"} <= set(lib.declared_symbols())
    h = lib.load()
    assert h.iir_abi_version() == 3
    assert lib.SIGNATURES["iir_image_metrics"][1][0] == ctypes.POINTER(lib.MetricsDesc)
    text = open(lib.HEADER_PATH).read()
    assert "iir_image_metrics(const iir_metrics_desc* d, void* stream)" in text and "#define IIR_METRICS_TILE 32" in text
    assert R.TILE == 32


def test_descriptor_layout_matches_header(tmp_path):
    import shutil
    import subprocess
    size = ctypes.sizeof(lib.MetricsDesc)
    assert size % 8 == 0 and lib.MetricsDesc.ws.offset % 8 == 0 and lib.MetricsDesc.out.offset == size - 8
    if shutil.which("gcc"):
        src = tmp_path / "sz.c"
        src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu %%zu %%zu %%zu", sizeof(iir_metrics_desc),'
                       'offsetof(iir_metrics_desc, what), offsetof(iir_metrics_desc, ws), offsetof(iir_metrics_desc, out));}' % lib.HEADER_PATH)
        subprocess.run(["gcc", str(src), "-o", str(tmp_path / "sz")], check=True)
        out = subprocess.run([str(tmp_path / "sz")], capture_output=True, text=True, check=True).stdout
        assert tuple(int(x) for x in out.split()) == (size, lib.MetricsDesc.what.offset, lib.MetricsDesc.ws.offset, lib.MetricsDesc.out.offset)


def test_invalid_arguments_are_rejected_without_a_gpu():
    h = lib.load()
    run = lambda d: h.iir_image_metrics(ctypes.byref(d), None)
    need = lambda d: h.iir_image_metrics_workspace_bytes(ctypes.byref(d))
    assert h.iir_image_metrics(None, None) == -1 and h.iir_image_metrics_workspace_bytes(None) == -1
    bad_geometry = [dict(N=0), dict(C=0), dict(H=0), dict(W=-3), dict(C=2), dict(C=4), dict(C=1, y_channel=1), dict(crop_border=-1),
                    dict(what=0), dict(what=4), dict(what=7), dict(H=32769), dict(W=40000),
                    dict(crop_border=16), dict(crop_border=20), dict(crop_border=11), dict(H=10), dict(W=10),
                    dict(what=lib.METRIC_SSIM, H=30, crop_border=10), dict(what=lib.METRIC_PSNR, crop_border=16),
                    dict(N=21846), dict(N=65536, y_channel=1), dict(N=65535, C=1, H=32768, W=32768, what=lib.METRIC_PSNR)]
    for kw in bad_geometry:
        assert run(_desc(**kw)) == -1 and need(_desc(**kw)) == -1, kw
    for kw in (dict(a=None), dict(b=None), dict(out=None), dict(ws=None), dict(ws=4100), dict(out=4097), dict(ws_bytes=0)):
        assert run(_desc(**kw)) == -1, kw
    # the workspace: two fp64 per workgroup -- a 22 x 30 map is one tile per plane; the MSE alone, one workgroup per 2048 elements
    assert need(_desc()) == 3 * 16 and need(_desc(y_channel=1)) == 16 and need(_desc(N=2, H=75, W=70, crop_border=4)) == 2 * 3 * 4 * 16
    assert need(_desc(H=43, W=44, C=1)) == 4 * 16 and need(_desc(H=42, W=42, C=1)) == 16
    assert need(_desc(what=lib.METRIC_PSNR)) == 2 * 16 and need(_desc(what=lib.METRIC_PSNR, H=8, W=8, crop_border=3)) == 16
    assert need(_desc(what=lib.METRIC_PSNR, crop_border=15, H=32, W=32)) == 16
    assert run(_desc(ws_bytes=47)) == -1
    if torch.cuda.is_available():      # on a GPU the next call would launch on address 4096
        return
    assert run(_desc(ws_bytes=48)) != -1                           # the valid descriptor passes validation (and fails at the launch)
