"""NIQE, the no-reference quality score of Mittal et al. 2013, for images that have no ground truth (an addition: the reference
reports no figures; the definitions are basicsr's `calculate_niqe`, which follows the MATLAB release; DESIGN.md section 7 "NIQE").

The device gives the per-block signed moments (`ops.niqe_stats`: grey, half-size image, MSCN, five maps, two scales); this
module does the rest in numpy fp64 -- the AGGD moment-matching fit, the 36 features per block, the Gaussian model and the
distance -- and owns the "pristine model", two small arrays:

    from instantir_amd.niqe import NIQE
    model = NIQE.from_file("niqe_pris_params.npz")        # basicsr's file as it is, or the MATLAB release's .mat
    model = NIQE.fit(clean_images); model.save("my.npz")  # or fitted from any set of clean images
    model(restored)                                       # fp64 array, one score per image; lower is better

    python -m instantir_amd.niqe fit CLEAN_DIR OUT.npz

There is no host path for the statistics: without the library and a GPU the calls raise.
"""
from __future__ import annotations

import math
import os
import warnings

import numpy as np

from .images import check_crop, dims, host_source, scoring_device

BLOCK = 96
NFEAT = 36
SHARPNESS_KEEP = 0.75

_TABLE = None


def _gamma(x):
    return np.vectorize(math.gamma, otypes=[np.float64])(x)


def _rho_table():
    """(alpha grid, rho(alpha) = Gamma(2/a)^2 / (Gamma(1/a) Gamma(3/a))), alpha = arange(0.2, 10.001, 0.001); rho is increasing."""
    global _TABLE
    if _TABLE is None:
        gam = np.arange(0.2, 10.001, 0.001)
        rec = np.reciprocal(gam)
        _TABLE = (gam, np.square(_gamma(rec * 2)) / (_gamma(rec) * _gamma(rec * 3)))
    return _TABLE


def aggd_from_sums(count_neg, count_pos, sumsq_neg, sumsq_pos, sumabs, n):
    """The asymmetric generalised Gaussian fit by moment matching from a sample's signed moments (arrays of one shape; `n` the
    number of elements): (alpha, beta_l, beta_r).  An empty side gives NaNs in all three."""
    gam, rho = _rho_table()
    cn, cp, qn, qp, ab = (np.asarray(v, dtype=np.float64) for v in (count_neg, count_pos, sumsq_neg, sumsq_pos, sumabs))
    with np.errstate(divide="ignore", invalid="ignore"):
        left, right = np.sqrt(qn / cn), np.sqrt(qp / cp)
        gammahat = left / right
        rhat = (ab / n) ** 2 / ((qn + qp) / n)
        rhatnorm = rhat * (gammahat ** 3 + 1) * (gammahat + 1) / (gammahat ** 2 + 1) ** 2
        ok = np.isfinite(rhatnorm)
        x = np.where(ok, rhatnorm, rho[0])
        hi = np.clip(np.searchsorted(rho, x), 1, len(rho) - 1)           # the nearest entry is hi - 1 or hi; the first on a tie
        pos = np.where((rho[hi - 1] - x) ** 2 <= (rho[hi] - x) ** 2, hi - 1, hi)
        alpha = np.where(ok, gam[pos], np.nan)
        a = np.where(ok, alpha, 1.0)
        scale = np.where(ok, np.sqrt(_gamma(1 / a) / _gamma(3 / a)), np.nan)
    return alpha, left * scale, right * scale


def features(stats):
    """fp64 (N, 2, nb, 26) from `ops.niqe_stats` (a tensor or an array) -> the NIQE features (N, nb, 36): 18 per scale, scale 1
    first; of v0 (alpha, (beta_l + beta_r) / 2), of each product map (alpha, mean, beta_l, beta_r)."""
    s = stats.detach().cpu().numpy() if hasattr(stats, "detach") else np.asarray(stats)
    s = s.astype(np.float64)
    if s.ndim != 4 or s.shape[1] != 2 or s.shape[3] != 26:
        raise ValueError(f"features: expected (N, 2, blocks, 26) statistics, got {s.shape}")
    out = np.empty(s.shape[:1] + (s.shape[2], NFEAT))
    for scale in range(2):
        n = float((BLOCK >> scale) ** 2)
        col = 18 * scale
        for q in range(5):
            v = s[:, scale, :, 5 * q:5 * q + 5]
            alpha, bl, br = aggd_from_sums(v[..., 0], v[..., 1], v[..., 2], v[..., 3], v[..., 4], n)
            if q == 0:
                out[:, :, col], out[:, :, col + 1] = alpha, (bl + br) / 2
                col += 2
            else:
                a = np.where(np.isfinite(alpha), alpha, 1.0)
                mean = (br - bl) * (_gamma(2 / a) / _gamma(1 / a))
                out[:, :, col], out[:, :, col + 1], out[:, :, col + 2], out[:, :, col + 3] = alpha, mean, bl, br
                col += 4
    return out


def sharpness(stats):
    """The mean sigma of every scale-1 block, (N, nb): what `fit` selects blocks by."""
    s = stats.detach().cpu().numpy() if hasattr(stats, "detach") else np.asarray(stats)
    return s[:, 0, :, 25].astype(np.float64) / float(BLOCK * BLOCK)


def gaussian_of(rows):
    """(nanmean over rows, sample covariance of the rows without NaN) of (rows, 36) features; NaNs with fewer than two finite rows."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, NFEAT)
    finite = rows[~np.isnan(rows).any(axis=1)]
    if len(finite) < 2:
        return np.full(NFEAT, np.nan), np.full((NFEAT, NFEAT), np.nan)
    with warnings.catch_warnings():                                  # a column that is NaN in every row has a NaN mean, quietly
        warnings.simplefilter("ignore", category=RuntimeWarning)
        mu = np.nanmean(rows, axis=0)
    return mu, np.cov(finite, rowvar=False)


def distance(mu_p, cov_p, mu_d, cov_d):
    """sqrt((mu_p - mu_d) pinv((cov_p + cov_d) / 2) (mu_p - mu_d)^T); NaN when either side holds a NaN."""
    d = np.asarray(mu_p, dtype=np.float64) - np.asarray(mu_d, dtype=np.float64)
    c = (np.asarray(cov_p, dtype=np.float64) + np.asarray(cov_d, dtype=np.float64)) / 2
    if np.isnan(d).any() or np.isnan(c).any():
        return float("nan")
    return float(np.sqrt(d @ np.linalg.pinv(c) @ d))


def _stats(who, images, crop_border, device):
    """-> (device statistics (N, 2, nb, 26), whether `images` was one image)."""
    from . import ops
    check_crop(who, crop_border)
    t, single = host_source(images, "images")
    N, C, H, W = dims(t)
    if C not in (1, 3):
        raise ValueError(f"{who}: images must have 1 or 3 channels, got {C}")
    nb = (max(H - 2 * crop_border, 0) // BLOCK) * (max(W - 2 * crop_border, 0) // BLOCK)
    if nb < 2:
        raise ValueError(f"{who}: {H}x{W} with crop_border {crop_border} holds {nb} block(s) of {BLOCK} x {BLOCK}; NIQE needs at "
                         "least two")
    return ops.niqe_stats(t.to(scoring_device(device, "instantir_amd.niqe")).contiguous(), crop_border=crop_border), single


class NIQE:
    """The pristine model (mu (36,), cov (36, 36), fp64) and the score against it."""

    def __init__(self, mu, cov):
        mu, cov = np.asarray(mu, dtype=np.float64), np.asarray(cov, dtype=np.float64)
        if mu.size != NFEAT or mu.ndim > 2 or cov.shape != (NFEAT, NFEAT):
            raise ValueError(f"NIQE: the model is a mean of {NFEAT} and a covariance of {NFEAT} x {NFEAT}, got {mu.shape} and {cov.shape}")
        self.mu, self.cov = mu.reshape(NFEAT).copy(), cov.copy()

    @classmethod
    def from_file(cls, path):
        """`.npz` with `mu_pris_param` / `cov_pris_param` (basicsr's niqe_pris_params.npz; other keys are ignored), or `.mat`
        with `mu_prisparam` / `cov_prisparam` (the MATLAB release's modelparameters.mat; needs scipy)."""
        ext = os.path.splitext(str(path))[1].lower()
        if ext == ".npz":
            with np.load(path) as f:
                keys, names = set(f.files), ("mu_pris_param", "cov_pris_param")
                data = {k: f[k] for k in names if k in keys}
        elif ext == ".mat":
            try:
                from scipy.io import loadmat
            except ImportError:
                raise ValueError(f"NIQE.from_file: reading {path} needs scipy (scipy.io.loadmat); convert it to .npz with "
                                 "mu_pris_param / cov_pris_param instead") from None
            f, names = loadmat(path), ("mu_prisparam", "cov_prisparam")
            data = {k: f[k] for k in names if k in f}
        else:
            raise ValueError(f"NIQE.from_file: {path} is neither .npz nor .mat")
        if len(data) != 2:
            raise ValueError(f"NIQE.from_file: {path} lacks {' / '.join(n for n in names if n not in data)}")
        mu, cov = (np.asarray(data[k]) for k in names)
        if mu.size != NFEAT or mu.ndim > 2 or cov.shape != (NFEAT, NFEAT):
            raise ValueError(f"NIQE.from_file: {path} holds {names[0]} {mu.shape} and {names[1]} {cov.shape}; expected {NFEAT} and "
                             f"{NFEAT} x {NFEAT}")
        return cls(mu, cov)

    def save(self, path):
        """The `.npz` form `from_file` reads."""
        np.savez(path, mu_pris_param=self.mu, cov_pris_param=self.cov)

    @classmethod
    def fit(cls, images, crop_border=0, device=None):
        """The model of a list of clean images (PIL images, arrays or tensors; sizes may differ, they go one at a time), as
        MATLAB's estimatemodelparam: of every image the blocks whose sharpness (mean sigma at scale 1) exceeds 0.75 of that
        image's sharpest; the kept rows of all images are pooled."""
        if not isinstance(images, (list, tuple)) or not images:
            raise ValueError("NIQE.fit: images must be a non-empty list")
        rows = []
        for im in images:
            stats, _ = _stats("NIQE.fit", im, crop_border, device)
            feats, sharp = features(stats), sharpness(stats)
            for f, s in zip(feats, sharp):
                rows.append(f[s > SHARPNESS_KEEP * s.max()])
        mu, cov = gaussian_of(np.concatenate(rows))
        if np.isnan(mu).any() or np.isnan(cov).any():
            raise ValueError("NIQE.fit: fewer than two blocks with finite features were kept")
        return cls(mu, cov)

    def score_features(self, feats):
        """(N, nb, 36) features -> fp64 (N,) scores."""
        return np.array([distance(self.mu, self.cov, *gaussian_of(f)) for f in feats], dtype=np.float64)

    def __call__(self, images, crop_border=0, device=None):
        """fp64 array of NIQE scores, one per image (the input kinds `metrics.psnr` accepts); NaN for an image with fewer than
        two blocks of finite features."""
        stats, _ = _stats("NIQE", images, crop_border, device)
        return self.score_features(features(stats))


def _main(argv=None):
    import argparse
    from PIL import Image
    p = argparse.ArgumentParser(prog="python -m instantir_amd.niqe", description="NIQE pristine models")
    sub = p.add_subparsers(dest="cmd", required=True)
    f = sub.add_parser("fit", help="fit a pristine model to the images of a directory")
    f.add_argument("clean_dir")
    f.add_argument("out")
    f.add_argument("--crop", type=int, default=0, help="border pixels dropped on every side")
    a = p.parse_args(argv)
    names = sorted(n for n in os.listdir(a.clean_dir) if n.lower().endswith((".png", ".jpg", ".jpeg", ".bmp", ".tif", ".tiff", ".webp")))
    if not names:
        raise SystemExit(f"{a.clean_dir} holds no image")
    try:
        model = NIQE.fit([Image.open(os.path.join(a.clean_dir, n)) for n in names], crop_border=a.crop)
    except ValueError as e:
        raise SystemExit(str(e))
    model.save(a.out)
    print(f"NIQE model of {len(names)} image(s) -> {a.out}")


if __name__ == "__main__":
    _main()
