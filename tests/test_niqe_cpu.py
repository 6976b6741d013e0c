"""CPU: the NIQE restatement (tests/niqe_ref.py) pinned to things independent of it -- scipy's convolution, a general restatement
of MATLAB's imresize, samples of a known generalised Gaussian, closed forms of the distance -- and the host side of the feature
held against the restatement: `instantir_amd.niqe` (features, model files, fit), the `infer` flag checks, the refusals of
`ops.niqe_stats` and of the C entry that need no GPU, and the gfx950 code objects of niqe.hip (no scratch)."""
import math
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

import niqe_ref as R
from instantir_amd import lib, niqe as NQ


# ---- the restatement against independent things --------------------------------------------------------------------------------
def test_taps_are_the_contracts():
    g = R.taps32()
    j = np.arange(7.0)
    want = np.exp(-((j - 3) ** 2) / (2 * (7 / 6) ** 2))
    assert g.dtype == np.float32 and np.array_equal(g, (want / want.sum()).astype(np.float32)) and np.array_equal(g, g[::-1])
    assert abs(float(g.astype(np.float64).sum()) - 1.0) < 4 * R.U
    assert R.HALF_TAPS.sum() == 1.0 and np.array_equal(R.HALF_TAPS.astype(np.float32).astype(np.float64), R.HALF_TAPS)


def test_window_equals_scipy_convolve_nearest():
    ndimage = pytest.importorskip("scipy.ndimage", reason="scipy is needed for the independent convolution")
    rng = np.random.default_rng(0)
    x = rng.uniform(0, 255, (37, 53))
    g = R.taps64()
    want = ndimage.convolve(x, np.outer(g, g), mode="nearest")
    assert np.abs(R._window(x, g) - want).max() < 1e-11
    m, sigma = R.mscn(x)
    mu = ndimage.convolve(x, np.outer(g, g), mode="nearest")
    s = np.sqrt(np.abs(ndimage.convolve(x * x, np.outer(g, g), mode="nearest") - mu * mu))
    assert np.abs(sigma - s).max() < 1e-9 and np.abs(m - (x - mu) / (s + 1)).max() < 1e-10


def _cubic(x):
    a = np.abs(x)
    return np.where(a <= 1, 1.5 * a ** 3 - 2.5 * a ** 2 + 1, np.where(a <= 2, -0.5 * a ** 3 + 2.5 * a ** 2 - 4 * a + 2, 0.0))


def _imresize_axis(x, scale, axis):
    """MATLAB's imresize along one axis: cubic a = -0.5, the kernel widened by 1 / scale (antialiasing), weights normalised per
    output sample, symmetric indices."""
    n = x.shape[axis]
    out_n = int(math.ceil(n * scale))
    width = 4.0 / scale
    u = (np.arange(out_n) + 1) / scale + 0.5 * (1 - 1 / scale)                    # 1-based centres
    left = np.floor(u - width / 2)
    P = int(math.ceil(width)) + 2
    idx = left[:, None] + np.arange(P)[None]
    w = scale * _cubic(scale * (u[:, None] - idx))
    w = w / w.sum(axis=1, keepdims=True)
    aux = np.concatenate([np.arange(n), np.arange(n - 1, -1, -1)])
    idx = aux[np.mod(idx.astype(np.int64) - 1, 2 * n)]
    x = np.moveaxis(x, axis, -1)
    out = (x[..., idx] * w).sum(-1)
    return np.moveaxis(out, -1, axis)


@pytest.mark.parametrize("shape", [(10, 14), (22, 6), (8, 8), (96, 192), (50, 34)])
def test_half_size_equals_general_imresize(shape):
    rng = np.random.default_rng(shape[0])
    x = np.floor(rng.uniform(0, 256, shape))
    want = _imresize_axis(_imresize_axis(x, 0.5, 0), 0.5, 1)
    got = R.half_size(x)
    assert got.shape == (shape[0] // 2, shape[1] // 2)
    assert np.abs(got - want).max() <= 1e-12 * 255


def _aggd_samples(alpha, beta_l, beta_r, n, seed):
    rng = np.random.default_rng(seed)
    mag = rng.gamma(1.0 / alpha, 1.0, n) ** (1.0 / alpha)
    left = rng.random(n) < beta_l / (beta_l + beta_r)
    return np.where(left, -beta_l * mag, beta_r * mag)


@pytest.mark.parametrize("alpha, beta_l, beta_r", [(0.8, 1.0, 1.0), (2.0, 1.2, 1.2), (2.0, 0.7, 1.3)])
def test_aggd_fit_recovers_a_known_generalised_gaussian(alpha, beta_l, beta_r):
    v = _aggd_samples(alpha, beta_l, beta_r, 10 ** 6, 7)
    for fitted in (R.aggd_of_samples(v),
                   tuple(float(t) for t in NQ.aggd_from_sums((v < 0).sum(), (v > 0).sum(), (v[v < 0] ** 2).sum(), (v[v > 0] ** 2).sum(),
                                                            np.abs(v).sum(), v.size))):
        a, bl, br = fitted
        assert abs(a - alpha) <= 0.02, fitted
        assert abs(bl - beta_l) <= 0.01 * beta_l and abs(br - beta_r) <= 0.01 * beta_r, fitted


def test_alpha_lookup_is_the_argmin_first_on_a_tie():
    gam, rho = NQ._rho_table()
    g2, r2 = R._rho()
    assert np.array_equal(gam, g2) and np.allclose(rho, r2, rtol=1e-14) and (np.diff(rho) > 0).all()
    rng = np.random.default_rng(1)
    xs = np.concatenate([rng.uniform(rho[0] - 0.01, rho[-1] + 0.01, 500), (rho[:-1] + rho[1:])[::400] / 2, rho[::977]])
    n = 1000.0
    for x in xs:                          # sums that give gammahat = 1 and rhatnorm = rhat = x
        ab = math.sqrt(x * n * n)
        alpha, _, _ = NQ.aggd_from_sums(np.array(500.0), np.array(500.0), np.array(n / 2), np.array(n / 2), np.array(ab), n)
        rn = (ab / n) ** 2 / 1.0
        assert float(alpha) == float(gam[int(np.argmin((rho - rn) ** 2))])


# ---- features, distance, the constant image --------------------------------------------------------------------------------------
def test_features_equal_the_restatements():
    u8 = R.picture(3, 2, 3, 200, 300)
    s = R.stats(u8)
    got, want = NQ.features(s), R.features(s)
    assert got.shape == (2, 6, 36) and got.dtype == np.float64
    assert np.array_equal(got[..., R.ALPHA_COLUMNS], want[..., R.ALPHA_COLUMNS])
    assert np.allclose(got, want, rtol=1e-13, atol=0)
    assert np.array_equal(NQ.features(torch.from_numpy(s)), got)
    assert np.allclose(NQ.sharpness(s), s[:, 0, :, 25] / 9216.0, rtol=0, atol=0)
    with pytest.raises(ValueError, match="features"):
        NQ.features(s[:, :1])


def test_constant_image_gives_nan_features_and_score():
    u8 = np.full((1, 96, 192, 1), 77, np.uint8)
    s = R.stats(u8)
    # the fp32 taps do not sum to 1 exactly, so m is a tiny constant and not 0: every map has one empty side all the same
    assert (np.minimum(s[..., 0:25:5], s[..., 1:25:5]) == 0).all() and (np.abs(s[..., 4:25:5]) < 0.1).all()
    assert np.isnan(NQ.features(s)).all() and np.isnan(R.features(s)).all()
    model = NQ.NIQE(np.zeros(36), np.eye(36))
    assert np.isnan(model.score_features(NQ.features(s))).all() and np.isnan(R.score((model.mu, model.cov), s)).all()


def test_distance_closed_forms():
    rng = np.random.default_rng(2)
    mu = rng.normal(size=36)
    A = rng.normal(size=(36, 36))
    cov = A @ A.T
    assert NQ.distance(mu, cov, mu, cov) == 0.0 and R.distance(mu, cov, mu, cov) == 0.0
    dp, dd, mu2 = rng.uniform(1, 2, 36), rng.uniform(1, 2, 36), rng.normal(size=36)
    want = math.sqrt((((mu - mu2) ** 2) / ((dp + dd) / 2)).sum())
    for dist in (NQ.distance, R.distance):
        assert abs(dist(mu, np.diag(dp), mu2, np.diag(dd)) - want) <= 1e-12 * want
    assert math.isnan(NQ.distance(mu, cov, np.full(36, np.nan), cov))
    rows = rng.normal(size=(50, 36))
    rows[3, 5] = np.nan
    m1, c1 = NQ.gaussian_of(rows)
    m2, c2 = R.gaussian_of(rows)
    assert np.allclose(m1, m2, rtol=1e-13) and np.allclose(c1, c2, rtol=1e-12, atol=1e-15)
    assert np.allclose(c1, np.cov(np.delete(rows, 3, axis=0), rowvar=False)) and m1[5] == pytest.approx(np.delete(rows[:, 5], 3).mean())
    assert np.isnan(NQ.gaussian_of(rows[3:5])[0]).all()           # one finite row


# ---- model files -----------------------------------------------------------------------------------------------------------------
def test_model_files(tmp_path):
    rng = np.random.default_rng(4)
    mu, A = rng.normal(size=36), rng.normal(size=(36, 36))
    cov = A @ A.T
    model = NQ.NIQE(mu, cov)
    model.save(str(tmp_path / "m.npz"))
    back = NQ.NIQE.from_file(str(tmp_path / "m.npz"))
    assert back.mu.tobytes() == mu.tobytes() and back.cov.tobytes() == cov.tobytes()
    np.savez(tmp_path / "basicsr.npz", mu_pris_param=mu[None], cov_pris_param=cov, something_else=np.zeros(3))     # (1, 36), as shipped
    assert np.array_equal(NQ.NIQE.from_file(str(tmp_path / "basicsr.npz")).mu, mu)
    np.savez(tmp_path / "short.npz", mu_pris_param=mu[:35], cov_pris_param=cov)
    np.savez(tmp_path / "wide.npz", mu_pris_param=mu, cov_pris_param=cov[:, :35])
    np.savez(tmp_path / "lacks.npz", mu_pris_param=mu)
    for bad, word in (("short.npz", "expected 36"), ("wide.npz", "expected 36"), ("lacks.npz", "lacks cov_pris_param")):
        with pytest.raises(ValueError, match=word):
            NQ.NIQE.from_file(str(tmp_path / bad))
    (tmp_path / "m.txt").write_text("x")
    with pytest.raises(ValueError, match="neither"):
        NQ.NIQE.from_file(str(tmp_path / "m.txt"))
    with pytest.raises(ValueError, match="NIQE"):
        NQ.NIQE(mu, cov[:35])


def test_mat_model_file(tmp_path):
    sio = pytest.importorskip("scipy.io", reason="scipy is needed to fabricate a .mat file")
    rng = np.random.default_rng(5)
    mu, cov = rng.normal(size=(1, 36)), rng.normal(size=(36, 36))
    sio.savemat(str(tmp_path / "modelparameters.mat"), {"mu_prisparam": mu, "cov_prisparam": cov})
    m = NQ.NIQE.from_file(str(tmp_path / "modelparameters.mat"))
    assert np.array_equal(m.mu, mu[0]) and np.array_equal(m.cov, cov)
    sio.savemat(str(tmp_path / "bad.mat"), {"mu_prisparam": mu[:, :30], "cov_prisparam": cov})
    with pytest.raises(ValueError, match="expected 36"):
        NQ.NIQE.from_file(str(tmp_path / "bad.mat"))


# ---- fit and the score, with the restatement standing in for the device -----------------------------------------------------------
@pytest.fixture
def host_stats(monkeypatch):
    from instantir_amd import ops
    calls = []

    def fake(src, crop_border=0, ws=None):
        calls.append(tuple(src.shape))
        return torch.from_numpy(R.stats(src.numpy(), crop_border))
    monkeypatch.setattr(ops, "niqe_stats", fake)
    return calls


def test_fit_is_the_pooled_definition_with_the_sharpness_rule(host_stats):
    from PIL import Image
    a = R.picture(11, 1, 1, 192, 288)                       # 2 x 3 blocks, textured
    b = R.picture(12, 1, 3, 300, 200, flat_rows=101)        # 3 x 2 blocks; the first row of blocks is flat
    model = NQ.NIQE.fit([a[0, :, :, 0], Image.fromarray(b[0])], device="cpu")
    assert host_stats == [(1, 192, 288, 1), (1, 300, 200, 3)]            # one at a time, uploaded as uint8
    rows, dropped = [], 0
    for im in (a, b):
        s = R.stats(im)
        f, sharp = R.features(s)[0], s[0, 0, :, 25] / 9216.0
        keep = sharp > 0.75 * sharp.max()
        dropped += int((~keep).sum())
        rows.append(f[keep])
    rows = np.concatenate(rows)
    assert dropped >= 2 and len(rows) >= 8                               # the rule drops the flat blocks
    assert np.allclose(model.mu, np.nanmean(rows, axis=0), rtol=1e-12)
    assert np.allclose(model.cov, np.cov(rows[~np.isnan(rows).any(1)], rowvar=False), rtol=1e-10, atol=1e-14)
    mu_r, cov_r = R.fit([R.stats(a), R.stats(b)])
    assert np.allclose(model.mu, mu_r, rtol=1e-12) and np.allclose(model.cov, cov_r, rtol=1e-10, atol=1e-14)
    with pytest.raises(ValueError, match="non-empty list"):
        NQ.NIQE.fit([], device="cpu")


def test_score_and_metrics_niqe_follow_the_restatement(host_stats):
    from instantir_amd import metrics as M
    clean = [R.stats(R.picture(s, 1, 1, 480, 576)) for s in (31, 32)]
    mu, cov = R.fit(clean)
    model = NQ.NIQE(mu, cov)
    u8 = R.picture(33, 2, 3, 209, 301)
    want = R.score((mu, cov), R.stats(u8, 4))
    got = model(u8, crop_border=4, device="cpu")
    assert got.dtype == np.float64 and got.shape == (2,) and (want > 0).all()
    assert np.allclose(got, want, rtol=1e-9)
    assert M.niqe(u8, model, crop_border=4, device="cpu") == got.tolist()
    one = M.niqe(u8[0], model, crop_border=4, device="cpu")
    assert isinstance(one, float) and one == got[0]
    assert M.niqe(torch.from_numpy(R.as_f32(u8)), model, crop_border=4, device="cpu") == got.tolist()
    for bad, word in ((dict(images=u8[:, :150, :150]), "at least two"), (dict(images=u8, crop_border=-1), "crop_border"),
                      (dict(images=np.zeros((200, 200, 2), np.uint8)), "1 or 3 channels")):
        with pytest.raises(ValueError, match=word):
            model(**bad, device="cpu")
    assert host_stats == [(2, 209, 301, 3), (2, 209, 301, 3), (1, 209, 301, 3), (2, 3, 209, 301)]     # refusals launch nothing


# ---- the CLI's flag checks --------------------------------------------------------------------------------------------------------
def test_apply_niqe_flag_checks(tmp_path):
    from instantir_amd.infer import apply_metrics, apply_niqe, build_niqe, build_parser
    params = tmp_path / "p.npz"
    NQ.NIQE(np.zeros(36), np.eye(36)).save(str(params))
    base = ["--test_path", "x"]
    parse = lambda *a: build_parser().parse_args(base + list(a))
    assert apply_niqe(parse()) is None and parse().niqe_path is None
    assert apply_niqe(parse("--niqe_path", str(params))) == {"path": str(params), "crop_border": 0, "input": False}
    args = parse("--niqe_path", str(params), "--metrics_crop", "4", "--input_fidelity")
    assert apply_niqe(args) == {"path": str(params), "crop_border": 4, "input": True}
    assert apply_metrics(parse("--niqe_path", str(params), "--metrics_crop", "4")) is None        # NIQE alone takes the crop
    with pytest.raises(SystemExit, match="--metrics_crop needs"):
        apply_metrics(parse("--metrics_crop", "4"))                                               # as before without the flag
    with pytest.raises(SystemExit, match="--metrics_y needs"):
        apply_metrics(parse("--niqe_path", str(params), "--metrics_y"))
    with pytest.raises(SystemExit, match="not a file"):
        apply_niqe(parse("--niqe_path", str(tmp_path / "missing.npz")))
    with pytest.raises(SystemExit, match="--metrics_crop must be >= 0"):
        apply_niqe(parse("--niqe_path", str(params), "--metrics_crop", "-1"))
    assert apply_niqe(types.SimpleNamespace()) is None
    (tmp_path / "junk.npz").write_bytes(b"not a zip")
    with pytest.raises(SystemExit, match="--niqe_path"):
        build_niqe({"path": str(tmp_path / "junk.npz")})
    assert np.array_equal(build_niqe({"path": str(params)}).cov, np.eye(36))


# ---- refusals that need no GPU ----------------------------------------------------------------------------------------------------
def test_ops_niqe_stats_refusals():
    from instantir_amd import ops
    z = torch.zeros
    for bad, word in ((z(1, 1, 96, 192, dtype=torch.float16), "contiguous 4-D"), (z(1, 96, 192), "contiguous 4-D"),
                      (z(1, 1, 96, 384)[:, :, :, ::2], "contiguous 4-D"), (np.zeros((1, 1, 96, 192), np.float32), "contiguous 4-D"),
                      (z(1, 2, 96, 192), "1 or 3 channels"), (z(1, 96, 192, 4, dtype=torch.uint8), "1 or 3 channels"),
                      (z(1, 1, 96, 191), "at least two"), (z(1, 1, 191, 191), "at least two"), (z(0, 1, 96, 192), "at least two"),
                      (z(1, 96, 192, 3, dtype=torch.uint8), "CUDA tensor")):
        with pytest.raises(ValueError, match=word):
            ops.niqe_stats(bad)
    for crop, word in ((-1, "crop_border"), (True, "crop_border"), (1.0, "crop_border"), (1, "at least two")):
        with pytest.raises(ValueError, match=word):
            ops.niqe_stats(z(1, 1, 96, 192), crop_border=crop)
    assert ops.NIQE_BLOCK == 96 and ops.NIQE_STATS == 26 and NQ.BLOCK == 96


def test_entry_refuses_bad_arguments_before_any_hip_call():
    h = lib.load()
    P = 4096
    ws_need = h.iir_niqe_workspace_bytes(2, 3, 209, 301, 0)
    assert ws_need == 2 * (192 * 288 + 96 * 144) * 4
    assert h.iir_niqe_workspace_bytes(1, 1, 300, 204, 5) == (288 * 192 + 144 * 96) * 4
    out_need = 2 * 2 * 6 * 26 * 8

    def call(src=P, u8=0, N=2, C=3, H=209, W=301, crop=0, ws=P, ws_bytes=ws_need, out=P, out_bytes=out_need):
        return h.iir_niqe_stats(src, u8, N, C, H, W, crop, ws, ws_bytes, out, out_bytes, None)
    for bad in (dict(src=None), dict(ws=None), dict(out=None), dict(N=0), dict(N=-1), dict(C=0), dict(H=0), dict(W=-5), dict(C=2), dict(C=4),
                dict(H=32769), dict(W=40000), dict(crop=-1), dict(crop=57), dict(H=95), dict(W=95), dict(N=65536, ws_bytes=1 << 40, out_bytes=1 << 40),
                dict(ws_bytes=ws_need - 1), dict(out_bytes=out_need - 8), dict(ws=P + 4), dict(out=P + 4)):
        assert call(**bad) == -1, bad
    for geo in ((0, 1, 96, 96, 0), (1, 2, 96, 96, 0), (1, 1, 95, 96, 0), (1, 1, 96, 96, 1), (1, 1, 96, 96, -1), (65536, 1, 96, 96, 0),
                (1, 1, 32769, 96, 0)):
        assert h.iir_niqe_workspace_bytes(*geo) == -1, geo
    assert h.iir_niqe_workspace_bytes(1, 1, 96, 96, 0) == (96 * 96 + 48 * 48) * 4       # one block is the entry's to take; ops refuses it
    assert h.iir_niqe_workspace_bytes(1, 3, 32768, 32768, 0) == (32736 * 32736 * 5 // 4) * 4


# ---- the code objects -------------------------------------------------------------------------------------------------------------
ROCM_LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")


def test_niqe_kernels_use_no_scratch_and_fit_static_lds(tmp_path):
    """{kernel: (private segment bytes, LDS bytes)} from the kernel metadata of the library's gfx950 code objects (the .hip_fatbin
    section holds one offload bundle per translation unit; each is unbundled on its own)."""
    tools = {t: os.path.join(ROCM_LLVM, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")}
    missing = [t for t, p in tools.items() if not os.path.exists(p)]
    if missing:
        pytest.skip(f"ROCm LLVM tools not found: {missing}")
    fat = tmp_path / "fat.bin"
    subprocess.run([tools["llvm-objcopy"], "--dump-section", f".hip_fatbin={fat}", lib.LIB_PATH, os.devnull], check=True, capture_output=True)
    data = fat.read_bytes()
    starts = [m.start() for m in re.finditer(re.escape(b"__CLANG_OFFLOAD_BUNDLE__"), data)]
    assert starts, "no offload bundle in .hip_fatbin"
    found = {}
    for i, s in enumerate(starts):
        piece, co = tmp_path / f"tu{i}.bundle", tmp_path / f"tu{i}.co"
        piece.write_bytes(data[s:starts[i + 1] if i + 1 < len(starts) else len(data)])
        r = subprocess.run([tools["clang-offload-bundler"], "--unbundle", "--type=o", f"--input={piece}", f"--output={co}",
                            "--targets=hipv4-amdgcn-amd-amdhsa--gfx950"], capture_output=True, text=True)
        if r.returncode != 0 or not co.exists() or co.stat().st_size == 0:
            continue
        notes = subprocess.run([tools["llvm-readelf"], "--notes", str(co)], capture_output=True, text=True, check=True).stdout
        for rec in re.split(r"\n\s*- \.", notes):
            name = re.search(r"\.name:\s+(\S+)", rec)
            priv = re.search(r"\.private_segment_fixed_size:\s+(\d+)", rec)
            lds = re.search(r"\.group_segment_fixed_size:\s+(\d+)", rec)
            if name and priv and lds and "niqe_" in name.group(1):
                found[name.group(1)] = (int(priv.group(1)), int(lds.group(1)))
    assert len(found) == 4 and sum("niqe_block_kernel" in k for k in found) == 2, sorted(found)
    assert all(priv == 0 and lds <= 64 * 1024 for priv, lds in found.values()), found
