"""CPU: the resampling contract (DESIGN.md section 7 "Resampling").  The fp64 restatement (tests/resample_ref.py) is tied to
its two oracles -- torch's antialiased interpolate for float mode, PIL for quantised mode -- the product's tables are tied
to the restatement, and the wrapper, pipeline and CLI checks are exercised without a GPU.

Bounds: restatement against torch 1e-9 of the 0..255 range (measured 4e-13: two fp64 evaluations of one definition);
against PIL at most 1 LSB on at most 3 % of the samples (PIL's 22-bit fixed-point coefficients; measured 1.55 % at worst,
bilinear 40x24 -> 163x99), exact at equal sizes; the GPU test's quantised inputs in the kernel's fp32 operation order
differ from the fp64 restatement on at most 0.5 % of the samples (the condition that test asserts on the device)."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import resample_ref as R


# ---- the restatement against its oracles ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bilinear", "bicubic"])
@pytest.mark.parametrize("geo", R.PIL_GEOMETRIES, ids=lambda g: f"{g[0][0]}x{g[0][1]}-{g[1][0]}x{g[1][1]}")
def test_float_mode_matches_torch_antialiased_interpolate(name, geo):
    (H, W), size = geo
    x = R.planar(R.noise_u8(3, 2, H, W, 3)).astype(np.float64)
    want = torch.nn.functional.interpolate(torch.from_numpy(x), size=size, mode=name, antialias=True, align_corners=False).numpy()
    err = np.abs(R.resize(x, size, name) - want).max()
    print(f"float {name} {H}x{W}->{size} max_abs_err {err:.3e}")
    assert err <= 1e-9 * 255


@pytest.mark.parametrize("name", R.FILTERS)
@pytest.mark.parametrize("geo", R.PIL_GEOMETRIES, ids=lambda g: f"{g[0][0]}x{g[0][1]}-{g[1][0]}x{g[1][1]}")
def test_quantised_mode_matches_pil(name, geo):
    (H, W), size = geo
    u8 = R.noise_u8(5, 1, H, W, 3)
    got = R.resize(R.planar(u8), size, name, quantize=True)[0].transpose(1, 2, 0)
    worst, frac = R.lsb_report(got, R.pil_resize(u8[0], size, name))
    print(f"quantised {name} {H}x{W}->{size} max_diff {worst:.0f} differing {100 * frac:.2f} %")
    assert worst <= 1 and frac <= 0.03


@pytest.mark.parametrize("name", R.FILTERS)
def test_equal_sizes_are_exact(name):
    u8 = R.noise_u8(6, 1, 37, 53, 3)
    got = R.resize(R.planar(u8), (37, 53), name, quantize=True)[0].transpose(1, 2, 0)
    assert np.array_equal(got, R.pil_resize(u8[0], (37, 53), name)) and np.array_equal(got, u8[0])


@pytest.mark.parametrize("name", R.FILTERS)
@pytest.mark.parametrize("geo", R.GPU_GEOMETRIES[:6], ids=lambda g: f"{g[0][0]}x{g[0][1]}-{g[1][0]}x{g[1][1]}")
def test_gpu_quantised_inputs_stay_inside_the_flip_budget_in_fp32_order(name, geo):
    """The rehearsal of test_resample_gpu's quantised cases: the same seeded inputs through the fp32-order restatement."""
    (H, W), size = geo
    x = R.planar(R.noise_u8(21, 2, H, W, 3))
    worst, frac = R.lsb_report(R.resize(x, size, name, quantize=True, fp32=True), R.resize(x, size, name, quantize=True))
    print(f"fp32-order {name} {H}x{W}->{size} max_diff {worst:.0f} differing {100 * frac:.3f} %")
    assert worst <= 1 and frac <= 0.005


# ---- the product's tables ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.FILTERS)
@pytest.mark.parametrize("n_in,n_out", [(53, 96), (96, 37), (300, 56), (24, 163), (1, 8), (7, 1), (1024, 224), (40, 40)])
def test_product_tables_equal_the_restatement(name, n_in, n_out):
    from instantir_amd import resample as RS
    bounds, weights = RS.coefficients(n_in, n_out, name)
    rows = R.taps(n_in, n_out, name)
    assert bounds.dtype == np.int32 and weights.dtype == np.float32 and bounds.shape == (n_out, 2) and weights.shape[0] == n_out
    L = max(np.abs(w).sum() for _, w in rows)
    for i, (lo, w) in enumerate(rows):
        assert (bounds[i, 0], bounds[i, 1]) == (lo, len(w)) and len(w) <= weights.shape[1]
        assert lo >= 0 and lo + len(w) <= n_in                      # every address the table names is inside the image
        assert np.array_equal(weights[i, :len(w)], w.astype(np.float32)), (i, weights[i], w)
        assert not weights[i, len(w):].any()                        # zero padding
        # n fp32 roundings of at most 2^-25 |w| each
        assert abs(weights[i].astype(np.float64).sum() - 1.0) <= L * 2.0 ** -24


def test_identity_table_and_filter_check():
    from instantir_amd import resample as RS
    b, w = RS.identity_tables(5)
    assert b.tolist() == [[i, 1] for i in range(5)] and w.tolist() == [[1.0]] * 5
    assert RS.FILTERS == ("bilinear", "bicubic", "lanczos")
    with pytest.raises(ValueError, match="filter"):
        RS.coefficients(4, 8, "nearest")
    with pytest.raises(ValueError, match="positive"):
        RS.coefficients(0, 8, "bilinear")


# ---- argument checks, no GPU ---------------------------------------------------------------------------------------------------
def test_ops_resample_checks_raise_before_any_launch():
    from instantir_amd import ops
    x = torch.zeros(1, 3, 8, 8)
    with pytest.raises(ValueError, match="filter must be one of"):
        ops.resample(x, (4, 4), "nearest")
    with pytest.raises(ValueError, match="size must be"):
        ops.resample(x, (4, 0))
    with pytest.raises(ValueError, match="size must be"):
        ops.resample(x, 4)
    with pytest.raises(ValueError, match="window .* does not lie inside"):
        ops.resample(x, (4, 4), window=(2, 0, 3, 4))
    with pytest.raises(ValueError, match="window must be"):
        ops.resample(x, (4, 4), window=(0, 0, 4))
    with pytest.raises(ValueError, match="lo <= hi"):
        ops.resample(x, (4, 4), clamp=(1.0, 0.0))
    with pytest.raises(ValueError, match="quantize must be a bool"):
        ops.resample(x, (4, 4), quantize=2)
    with pytest.raises(ValueError, match="contiguous 4-D tensor"):
        ops.resample(x.half(), (4, 4))
    with pytest.raises(ValueError, match="contiguous 4-D tensor"):
        ops.resample(x[0], (4, 4))
    with pytest.raises(ValueError, match="contiguous 4-D tensor"):
        ops.resample(x.permute(0, 1, 3, 2)[:, :, :, :4], (4, 4))
    with pytest.raises(ValueError, match="out must be"):
        ops.resample(x, (4, 4), out=torch.zeros(1, 3, 4, 5))
    with pytest.raises(ValueError, match="out overlaps src"):
        ops.resample(x, (8, 8), out=x)
    with pytest.raises(ValueError, match="CUDA tensor"):
        ops.resample(x, (4, 4))
    with pytest.raises(ValueError, match="CUDA tensor"):
        ops.resample(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), (4, 4), quantize=True)


def test_pipeline_resize_argument_checks():
    from instantir_amd.pipeline import InstantIRPipeline as P
    sig = inspect.signature(P.__call__).parameters
    assert sig["work_size"].default is None and sig["output_size"].default is None and sig["resample"].default == "bilinear"
    assert all(k in P.__call__.__doc__ for k in ("work_size", "output_size", "resample"))
    assert P._check_resize(None, None, "bilinear", "pil") == (None, None)
    assert P._check_resize((64, 128), [30, 20], "lanczos", "pil") == ((64, 128), (30, 20))
    with pytest.raises(ValueError, match="resample must be one of"):
        P._check_resize((64, 64), None, "nearest", "pil")
    with pytest.raises(ValueError, match="needs work_size or output_size"):
        P._check_resize(None, None, "bicubic", "pil")
    with pytest.raises(ValueError, match="work_size .* multiple of 8"):
        P._check_resize((64, 60), None, "bilinear", "pil")
    with pytest.raises(ValueError, match="work_size must be"):
        P._check_resize((64,), None, "bilinear", "pil")
    with pytest.raises(ValueError, match="output_size must be"):
        P._check_resize(None, (0, 5), "bilinear", "pil")
    with pytest.raises(ValueError, match="LQ latent"):
        P._check_resize((64, 64), None, "bilinear", "pil", torch.zeros(1, 4, 8, 8))
    with pytest.raises(ValueError, match="output_type='latent'"):
        P._check_resize(None, (64, 64), "bilinear", "latent")


def test_preprocess_geometry_and_host_form_refuses_tensors():
    from instantir_amd import encoders as E
    assert E._preprocess_geometry(300, 200, 256, 224) == ((256, 384), (16, 80, 224, 224))
    assert E._preprocess_geometry(47, 61, 224, 224) == ((291, 224), (33, 0, 224, 224))
    with pytest.raises(ValueError, match="device="):
        E.dinov2_preprocess(torch.zeros(1, 3, 8, 8))
    assert inspect.signature(E.dinov2_preprocess).parameters["device"].default is None
    assert inspect.signature(E.clip_preprocess).parameters["device"].default is None


def test_as_batch_keeps_eight_bit_images_eight_bit():
    from PIL import Image
    from instantir_amd import resample as RS
    u8 = R.noise_u8(1, 2, 5, 7, 3)
    b, kind = RS.as_batch([Image.fromarray(u8[0]), Image.fromarray(u8[1])])
    assert kind == "u8" and b.dtype == np.uint8 and np.array_equal(b, u8)
    b, kind = RS.as_batch(u8)
    assert kind == "u8" and b.shape == (2, 5, 7, 3)
    b, kind = RS.as_batch(Image.fromarray(u8[0, :, :, 0]))
    assert kind == "u8" and b.shape == (1, 5, 7, 1)
    t, kind = RS.as_batch(torch.rand(3, 5, 7))
    assert kind == "f32" and t.shape == (1, 3, 5, 7)
    with pytest.raises(ValueError, match="share one size"):
        RS.as_batch([u8[0], u8[1, :4]])


# ---- CLI ---------------------------------------------------------------------------------------------------------------------------
def test_cli_flags():
    import instantir_amd.infer as cli
    p = cli.build_parser()
    a = p.parse_args(["--test_path", "x"])
    assert a.device_resize is False and a.resample is None and cli.apply_device_resize(None, a) == (False, "bilinear")
    a = p.parse_args(["--test_path", "x", "--device_resize"])
    assert cli.apply_device_resize(None, a) == (True, "bilinear")
    a = p.parse_args(["--test_path", "x", "--device_resize", "--resample", "lanczos"])
    assert cli.apply_device_resize(None, a) == (True, "lanczos")
    with pytest.raises(SystemExit, match="--resample needs --device_resize"):
        cli.apply_device_resize(None, p.parse_args(["--test_path", "x", "--resample", "bicubic"]))
    with pytest.raises(SystemExit):
        p.parse_args(["--test_path", "x", "--device_resize", "--resample", "nearest"])

    class Pipe:
        on = False

        def enable_device_preprocess(self):
            self.on = True
    pipe = Pipe()
    cli.apply_device_resize(pipe, p.parse_args(["--test_path", "x", "--device_resize"]))
    assert pipe.on


def test_resize_plan_is_resize_img_without_the_resize():
    from PIL import Image
    import instantir_amd.infer as cli
    for (w, h), kw in (((300, 200), {}), ((2000, 900), {}), ((640, 480), dict(width=1200)), ((640, 480), dict(width=500, height=700))):
        im, out = cli.resize_img(Image.new("RGB", (w, h)), **kw)
        assert cli.resize_plan((w, h), **kw) == (im.size, out)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_library_exports_and_lib_declares_the_new_entry():
    from instantir_amd import lib
    assert "iir_resample_pass" in lib.declared_symbols() and "iir_resample_pass" in lib.SIGNATURES
    assert hasattr(ctypes.CDLL(lib.LIB_PATH), "iir_resample_pass")
    # the descriptor as a C compiler lays it out: natural alignment, 8-byte pointers
    assert ctypes.sizeof(lib.ResampleDesc) == 120
    assert lib.ResampleDesc.dst.offset == 16 and lib.ResampleDesc.bounds.offset == 48 and lib.ResampleDesc.scale.offset == 104


def test_invalid_arguments_are_rejected_without_a_gpu():
    """Every IIR_EINVAL of iir_resample_pass comes back before any HIP call, so it can be provoked here with made-up addresses."""
    from instantir_amd import lib
    fn = ctypes.CDLL(lib.LIB_PATH).iir_resample_pass
    fn.restype, fn.argtypes = lib.SIGNATURES["iir_resample_pass"]

    def desc(**kw):
        d = lib.ResampleDesc()
        d.src, d.dst, d.bounds, d.weights = 0x10000000, 0x20000000, 0x30000000, 0x40000000
        d.N, d.C, d.H, d.W, d.axis, d.out_size, d.ksize = 1, 3, 8, 8, 0, 4, 5
        d.y0, d.x0, d.h, d.w = 0, 0, 8, 4
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    assert fn(None, None) == -1
    bad = [dict(src=None), dict(dst=None), dict(bounds=None), dict(weights=None), dict(N=0), dict(C=-1), dict(H=0), dict(W=0),
           dict(out_size=0), dict(ksize=0), dict(axis=2), dict(H=32769), dict(out_size=32769, w=32769), dict(N=65536, C=1),
           dict(y0=-1), dict(x0=1), dict(h=9), dict(w=0), dict(w=5), dict(clamp=1, lo=1.0, hi=0.0), dict(clamp=1, lo=float("nan"), hi=0.0),
           dict(dst=0x10000000), dict(dst=0x10000000 + 8 * 8 * 3 * 4 - 4), dict(src=0x20000000 + 4, src_u8=1)]
    for kw in bad:
        assert fn(ctypes.byref(desc(**kw)), None) == -1, kw
    # a vertical launch counts its window rows against out_size and its columns against W
    assert fn(ctypes.byref(desc(axis=1, h=5, w=8)), None) == -1
    assert fn(ctypes.byref(desc(axis=1, h=4, w=9)), None) == -1
