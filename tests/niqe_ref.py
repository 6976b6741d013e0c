"""Restatements of the NIQE contract (DESIGN.md section 7 "NIQE"; include/instantir_hip.h: iir_niqe_stats).

`stats`      -- fp64 numpy, the contract as written: grey, block grid, half-size image, MSCN, the five maps of every block and
                their 26 sums.  `features`, `gaussian_of`, `distance`, `score` and `fit` finish it: everything in this file
                is independent of instantir_amd/niqe.py, which the tests hold against it.  The judge of the kernel.
`stats32`    -- the same sums with fp32 rounding wherever the kernel rounds: the pixel pipeline, the 8-tap and 7-tap fmaf chains
                in index order, the moments about 128, m, the products, every thread's own sum of B * B / 384 terms; fp64 from
                there.  `maps` / `maps32` expose m and sigma per scale for the element error bound b.
Sources are what the kernel takes: uint8 (N, H, W, C), or float32 (N, C, H, W) on a [0, 1] scale.

The one thing the contract leaves open is the rounding of a grey value that sits on a half: Y of an RGB pixel is formed in fp32 by
the kernel and in fp64 here, so `picture` keeps every pixel's exact Y at least HALF_MARGIN away from a half (it moves the blue
channel of a pixel that is not), and both then round to the same integer.
"""
import math

import numpy as np

BLOCK = 96
NSTAT = 26
NT = 384                       # threads of a block's workgroup: a thread owns the rows tr + k * (NT / B) of one column
PIVOT = 128.0
U = 2.0 ** -24
HALF_TAPS = np.array([-3, -9, 29, 111, 111, 29, -9, -3], dtype=np.float64) / 256.0
SHIFTS = ((0, 1), (1, 0), (1, 1), (1, -1))
# |fp32 Y - exact Y| <= (7 * 219 + 235) U + 3 * 255 U * 0.51 ~ 1.3e-4 (metrics_ref.pixel_error plus an fp32 source's x 255)
HALF_MARGIN = 2.5e-4

# (N, C, H, W), crop_border: two blocks and one seam; Y, 2 x 3 blocks, ragged, two images; a crop, then 290 x 194 = 3 x 2 blocks; uint8
GPU_SHAPES = [((1, 1, 96, 192), 0), ((2, 3, 209, 301), 0), ((1, 3, 300, 204), 5), ((1, 1, 192, 192), 0)]


def taps32():
    j = np.arange(7, dtype=np.float64)
    g = np.exp(-((j - 3.0) ** 2) / (2.0 * (7.0 / 6.0) ** 2))
    return (g / g.sum()).astype(np.float32)


def taps64():
    """The contract's window: the fp32-rounded taps, as fp64 numbers."""
    return taps32().astype(np.float64)


# ---- seeded sources ---------------------------------------------------------------------------------------------------------
def _smooth(x, passes):
    for _ in range(passes):
        x = (np.roll(x, 1, -1) + 2 * x + np.roll(x, -1, -1)) / 4
        x = (np.roll(x, 1, -2) + 2 * x + np.roll(x, -1, -2)) / 4
    return x


def _luma_exact(u8):
    """Y of uint8 (..., 3) in fp64."""
    r, g, b = (u8[..., i].astype(np.float64) for i in range(3))
    return 16.0 + (65.481 * r + 128.553 * g + 24.966 * b) / 255.0


def picture(seed, N, C, H, W, flat_rows=0):
    """Filtered noise as uint8 (N, H, W, C) with every value in [0, 250]: natural-scene statistics need texture at every scale, so
    noise smoothed a little, plus noise smoothed a lot.  Rows [0, flat_rows) are constant.  For C = 3 every pixel's Y stays
    HALF_MARGIN away from a half (see the module docstring)."""
    rng = np.random.default_rng(seed)
    fine = _smooth(rng.normal(0, 1, (N, C, H, W)), 1)
    coarse = _smooth(rng.normal(0, 1, (N, C, H, W)), 6)
    x = 125.0 + 60.0 * fine / fine.std() + 40.0 * coarse / coarse.std()
    x[:, :, :flat_rows] = 97.0
    u8 = np.ascontiguousarray(np.clip(np.floor(x + 0.5), 0, 250).astype(np.uint8).transpose(0, 2, 3, 1))
    if C == 3:
        for _ in range(8):
            y = _luma_exact(u8)
            near = np.abs(y - np.floor(y) - 0.5) < HALF_MARGIN
            if not near.any():
                break
            u8[..., 2] = np.where(near, np.where(u8[..., 2] < 250, u8[..., 2] + 1, u8[..., 2] - 1), u8[..., 2])
        assert not near.any()
    return u8


def as_f32(u8):
    """uint8 (N, H, W, C) -> the fp32 planar form of the same content, (N, C, H, W) on [0, 1]."""
    return np.ascontiguousarray((u8.astype(np.float32) / np.float32(255.0)).transpose(0, 3, 1, 2))


def grid(H, W, crop):
    return (H - 2 * crop) // BLOCK, (W - 2 * crop) // BLOCK


# ---- fp64 ----------------------------------------------------------------------------------------------------------------------
def grey(x, crop_border=0):
    """The rounded grey block-grid image, fp64 (N, 96 nbh, 96 nbw)."""
    x = np.asarray(x)
    if x.dtype == np.uint8:
        p = x.transpose(0, 3, 1, 2).astype(np.float64)
    else:
        assert x.dtype == np.float32
        p = x.astype(np.float64) * 255.0
    N, C, H, W = p.shape
    c = crop_border
    p = p[:, :, c:H - c, c:W - c]
    nbh, nbw = grid(H, W, c)
    p = p[:, :, :BLOCK * nbh, :BLOCK * nbw]
    v = 16.0 + (65.481 * p[:, 0] + 128.553 * p[:, 1] + 24.966 * p[:, 2]) / 255.0 if C == 3 else p[:, 0]
    return np.clip(np.floor(v + 0.5), 0.0, 255.0)


def _sym(i, n):
    return np.where(i < 0, -1 - i, np.where(i >= n, 2 * n - 1 - i, i))


def half_size(g):
    """MATLAB's imresize(g, 0.5) for even sides: the 8-tap filter along y, then along x, at symmetric indices."""
    H, W = g.shape[-2:]
    rows = _sym(2 * np.arange(H // 2)[:, None] - 3 + np.arange(8)[None], H)
    t = sum(HALF_TAPS[j] * g[..., rows[:, j], :] for j in range(8))
    cols = _sym(2 * np.arange(W // 2)[:, None] - 3 + np.arange(8)[None], W)
    return sum(HALF_TAPS[i] * t[..., :, cols[:, i]] for i in range(8))


def _window(x, g):
    """G * x with replicate padding at the edge of x, along x then y."""
    H, W = x.shape[-2:]
    p = np.pad(x, [(0, 0)] * (x.ndim - 2) + [(3, 3), (3, 3)], mode="edge")
    h = sum(g[j] * p[..., :, j:j + W] for j in range(7))
    return sum(g[j] * h[..., j:j + H, :] for j in range(7))


def mscn(x):
    """(m, sigma) of a plane (..., H, W), fp64."""
    g = taps64()
    mu = _window(x, g)
    sigma = np.sqrt(np.abs(_window(x * x, g) - mu * mu))
    return (x - mu) / (sigma + 1.0), sigma


def maps(x, crop_border=0):
    """[(m, sigma) at scale 1, (m, sigma) at scale 2] of the block-grid image, fp64."""
    g = grey(x, crop_border)
    return [mscn(g), mscn(half_size(g))]


def _blocks(a, B):
    """(N, nbh B, nbw B) -> (N, nb, B, B), blocks in raster order."""
    N, H, W = a.shape
    return a.reshape(N, H // B, B, W // B, B).transpose(0, 1, 3, 2, 4).reshape(N, -1, B, B)


def block_maps(m):
    """(N, nb, B, B) -> (5, N, nb, B, B): v0 = m, v1..v4 = m roll(m, s) within the block."""
    return np.stack([m] + [m * np.roll(m, s, axis=(-2, -1)) for s in SHIFTS])


def stats(x, crop_border=0):
    """fp64 (N, 2, nb, 26): the contract's sums."""
    out = []
    for scale, (m, sigma) in enumerate(maps(x, crop_border)):
        B = BLOCK >> scale
        v = block_maps(_blocks(m, B))
        neg, pos = v < 0, v > 0
        five = np.stack([neg.sum((-2, -1)), pos.sum((-2, -1)), (v * v * neg).sum((-2, -1)), (v * v * pos).sum((-2, -1)),
                         np.abs(v).sum((-2, -1))], axis=-1).astype(np.float64)                      # (5 maps, N, nb, 5)
        s = np.concatenate([five.transpose(1, 2, 0, 3).reshape(five.shape[1], five.shape[2], 25),
                            _blocks(sigma, B).sum((-2, -1))[..., None]], axis=-1)
        out.append(s)
    return np.stack(out, axis=1)


_RHO = None


def _rho():
    global _RHO
    if _RHO is None:
        gam = np.arange(0.2, 10.001, 0.001)
        G = np.vectorize(math.gamma)
        _RHO = (gam, G(2 / gam) ** 2 / (G(1 / gam) * G(3 / gam)))
    return _RHO


def aggd(cn, cp, qn, qp, ab, n):
    """(alpha, beta_l, beta_r) of one sample from its signed moments, as the contract words it; NaNs for an empty side."""
    if cn == 0 or cp == 0:
        return (math.nan,) * 3
    gam, rho = _rho()
    left, right = math.sqrt(qn / cn), math.sqrt(qp / cp)
    gh = left / right
    rhat = (ab / n) ** 2 / ((qn + qp) / n)
    rn = rhat * (gh ** 3 + 1) * (gh + 1) / (gh ** 2 + 1) ** 2
    alpha = float(gam[int(np.argmin((rho - rn) ** 2))])
    k = math.sqrt(math.gamma(1 / alpha) / math.gamma(3 / alpha))
    return alpha, left * k, right * k


def aggd_of_samples(v):
    v = np.asarray(v, dtype=np.float64).ravel()
    return aggd((v < 0).sum(), (v > 0).sum(), (v[v < 0] ** 2).sum(), (v[v > 0] ** 2).sum(), np.abs(v).sum(), v.size)


def features(s):
    """(N, 2, nb, 26) -> (N, nb, 36)."""
    N, _, nb, _ = s.shape
    out = np.empty((N, nb, 36))
    for n in range(N):
        for b in range(nb):
            row = []
            for scale in range(2):
                cnt = float((BLOCK >> scale) ** 2)
                for q in range(5):
                    alpha, bl, br = aggd(*s[n, scale, b, 5 * q:5 * q + 5], cnt)
                    if q == 0:
                        row += [alpha, (bl + br) / 2]
                    else:
                        mean = (br - bl) * math.gamma(2 / alpha) / math.gamma(1 / alpha) if alpha == alpha else math.nan
                        row += [alpha, mean, bl, br]
            out[n, b] = row
    return out


ALPHA_COLUMNS = [c for s in (0, 18) for c in (s, s + 2, s + 6, s + 10, s + 14)]


def gaussian_of(rows):
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 36)
    finite = rows[~np.isnan(rows).any(axis=1)]
    if len(finite) < 2:
        return np.full(36, np.nan), np.full((36, 36), np.nan)
    cols = [rows[:, c][~np.isnan(rows[:, c])] for c in range(36)]
    mu = np.array([c.mean() if len(c) else np.nan for c in cols])
    d = finite - finite.mean(axis=0)
    return mu, d.T @ d / (len(finite) - 1)


def distance(mu_p, cov_p, mu_d, cov_d):
    d = mu_p - mu_d
    c = (cov_p + cov_d) / 2
    if np.isnan(d).any() or np.isnan(c).any():
        return math.nan
    return math.sqrt(d @ np.linalg.pinv(c) @ d)


def score(model, s):
    """(N,) scores of statistics `s` under model = (mu_p, cov_p)."""
    return np.array([distance(model[0], model[1], *gaussian_of(f)) for f in features(s)])


def fit(stat_list):
    """The pooled model of a list of per-image statistics (1, 2, nb, 26): the 0.75 sharpness rule per image."""
    rows = []
    for s in stat_list:
        for f, sg in zip(features(s), s[:, 0, :, 25] / float(BLOCK * BLOCK)):
            rows.append(f[sg > 0.75 * sg.max()])
    return gaussian_of(np.concatenate(rows))


# ---- fp32, rounded where the kernel rounds --------------------------------------------------------------------------------------
def _fma32(g, v, acc):
    """fmaf through long double (metrics_ref._fma32): differs from fmaf only within 2^-40 of an fp32 tie."""
    return (np.longdouble(g) * v.astype(np.longdouble) + acc.astype(np.longdouble)).astype(np.float32)


def grey32(x, crop_border=0):
    f = np.float32
    x = np.asarray(x)
    p = x.transpose(0, 3, 1, 2).astype(np.float32) if x.dtype == np.uint8 else x * f(255.0)
    N, C, H, W = p.shape
    c = crop_border
    nbh, nbw = grid(H, W, c)
    p = p[:, :, c:c + BLOCK * nbh, c:c + BLOCK * nbw]
    if C == 3:
        t = f(65.481) * p[:, 0]
        t = t + f(128.553) * p[:, 1]
        t = t + f(24.966) * p[:, 2]
        v = f(16.0) + t / f(255.0)
    else:
        v = p[:, 0]
    return np.clip(np.floor(v + f(0.5)), f(0.0), f(255.0)).astype(np.float32)


def half_size32(g):
    H, W = g.shape[-2:]
    w = HALF_TAPS.astype(np.float32)
    rows = _sym(2 * np.arange(H // 2)[:, None] - 3 + np.arange(8)[None], H)
    t = np.zeros(g.shape[:-2] + (H // 2, W), np.float32)
    for j in range(8):
        t = _fma32(w[j], g[..., rows[:, j], :], t)
    cols = _sym(2 * np.arange(W // 2)[:, None] - 3 + np.arange(8)[None], W)
    out = np.zeros(g.shape[:-2] + (H // 2, W // 2), np.float32)
    for i in range(8):
        out = _fma32(w[i], t[..., :, cols[:, i]], out)
    return out


def _window32(x):
    g = taps32()
    H, W = x.shape[-2:]
    p = np.pad(x, [(0, 0)] * (x.ndim - 2) + [(3, 3), (3, 3)], mode="edge")
    h = np.zeros(p.shape[:-1] + (W,), np.float32)
    for j in range(7):
        h = _fma32(g[j], p[..., :, j:j + W], h)
    out = np.zeros(x.shape, np.float32)
    for j in range(7):
        out = _fma32(g[j], h[..., j:j + H, :], out)
    return out


def mscn32(x):
    a = x - np.float32(PIVOT)
    mu = _window32(a)
    sigma = np.sqrt(np.abs(_window32(a * a) - mu * mu))
    return (a - mu) / (sigma + np.float32(1.0)), sigma


def maps32(x, crop_border=0):
    g = grey32(x, crop_border)
    return [mscn32(g), mscn32(half_size32(g))]


def _thread_sums(v, B):
    """(..., B, B) fp32 -> fp64 (...): a thread adds rows tr, tr + ROWS, ... of its column in fp32 from 0; fp64 over threads."""
    rows = NT // B
    per = v.reshape(v.shape[:-2] + (B // rows, rows, B))
    acc = np.zeros(per.shape[:-3] + (rows, B), np.float32)
    for k in range(B // rows):
        acc = acc + per[..., k, :, :]
    return acc.astype(np.float64).sum((-2, -1))


def stats32(x, crop_border=0):
    out = []
    zero = np.float32(0.0)
    for scale, (m, sigma) in enumerate(maps32(x, crop_border)):
        B = BLOCK >> scale
        v = block_maps(_blocks(m, B))
        assert v.dtype == np.float32
        neg, pos = v < 0, v > 0
        q = v * v
        five = np.stack([neg.sum((-2, -1)).astype(np.float64), pos.sum((-2, -1)).astype(np.float64),
                         _thread_sums(np.where(neg, q, zero), B), _thread_sums(np.where(pos, q, zero), B),
                         _thread_sums(np.abs(v), B)], axis=-1)
        s = np.concatenate([five.transpose(1, 2, 0, 3).reshape(five.shape[1], five.shape[2], 25),
                            _thread_sums(_blocks(sigma, B), B)[..., None]], axis=-1)
        out.append(s)
    return np.stack(out, axis=1)


# ---- the element error bound and what follows from it ---------------------------------------------------------------------------
def element_gaps(x, crop_border=0):
    """(max |m32 - m64|, max |sigma32 - sigma64|) over both scales of one source: the CPU rounding model's gap."""
    gm = gs = 0.0
    for (m, s), (m32, s32) in zip(maps(x, crop_border), maps32(x, crop_border)):
        gm = max(gm, float(np.abs(m32.astype(np.float64) - m).max()))
        gs = max(gs, float(np.abs(s32.astype(np.float64) - s).max()))
    return gm, gs


def sum_bounds(x, crop_border, b, b_sigma):
    """The bound on |kernel sum - fp64 sum| for every entry of `stats`, (N, 2, nb, 26), from the element bounds b (of m) and
    b_sigma (DESIGN.md section 7 "NIQE"), and the number of elements of every block and map that may change side, (N, 2, nb, 5):
      b_v = b for v0, 2 b max|m| for a product (max over the scale's image);
      sum of v^2 over one side: sum over the block of (2 |v| b_v + b_v^2) -- an element that changes side has |v| <= b_v and is
          inside that -- plus 26 U sum v^2 for the fp32 square and a thread's 24-term sum;
      sum of |v|: n b_v + 25 U sum |v|;   sum of sigma: n b_sigma + 25 U sum sigma;
      counts: at most the number of elements with |v| <= b_v."""
    bounds, flips = [], []
    for scale, (m, sigma) in enumerate(maps(x, crop_border)):
        B = BLOCK >> scale
        n = float(B * B)
        v = block_maps(_blocks(m, B))
        bv = np.array([b] + [2 * b * float(np.abs(m).max())] * 4).reshape(5, 1, 1)
        sa, sq = np.abs(v).sum((-2, -1)), (v * v).sum((-2, -1))                                      # (5, N, nb)
        flip = (np.abs(v) <= bv[..., None, None]).sum((-2, -1))
        t_sq = 2 * bv * sa + n * bv * bv + 26 * U * sq
        t_ab = n * bv + 25 * U * sa
        five = np.stack([flip, flip, t_sq, t_sq, t_ab], axis=-1).astype(np.float64)
        ssum = _blocks(sigma, B).sum((-2, -1))
        bounds.append(np.concatenate([five.transpose(1, 2, 0, 3).reshape(five.shape[1], five.shape[2], 25),
                                      (n * b_sigma + 25 * U * ssum)[..., None]], axis=-1))
        flips.append(flip.transpose(1, 2, 0))
    return np.stack(bounds, axis=1), np.stack(flips, axis=1)
