"""Restatements of the image-metrics contract (DESIGN.md section 7 "Image metrics"; include/instantir_hip.h: iir_image_metrics).

`evaluate`   -- fp64 numpy, the contract as written: sources to 0..255 units, crop, Y, MSE, the 11 x 11 Gaussian-window SSIM
                over the positions at which the window lies inside the image.  The judge of the kernel.
`evaluate32` -- the same figures with fp32 rounding wherever the kernel rounds: the pixel pipeline in fp32, the moments about
                128 as two chains of 11 fmaf in index order, the map in the kernel's operation order, every thread's own
                few-term fp32 sum, fp64 from there.  It shows slips far below the worst-case bound.
`bounds`     -- the worst-case distance between the two, derived from the rounding points (the derivation is in DESIGN.md).
Sources are what the kernel takes: uint8 (N, H, W, C), or float32 (N, C, H, W) on a [0, 1] scale.
"""
import numpy as np

WIN = 11
TILE = 32                      # IIR_METRICS_TILE
PIVOT = 128.0
C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
U = 2.0 ** -24
NT, STAGE, PE = 256, 7, 8      # threads per workgroup; staged pixels per thread; pixels per thread of the MSE-only launch

# (N, C, H, W), crop_border: one window; one tile edge crossed in x, ragged, two images; both axes crossed with the halo of a
# second tile; a crop that is a multiple of nothing (T = 32)
GPU_SHAPES = [((1, 3, 11, 11), 0), ((2, 3, 12, 45), 0), ((1, 1, 43, 44), 0), ((1, 3, 75, 70), 4)]
# source forms: (a is uint8, b is uint8, quantize)
SOURCE_FORMS = {"u8_u8": (True, True, (False, False)), "f32q_u8": (False, True, (True, False)),
                "f32_u8": (False, True, (False, False)), "f32_f32": (False, False, (False, False))}


def taps64():
    j = np.arange(WIN, dtype=np.float64)
    g = np.exp(-((j - 5.0) ** 2) / (2.0 * 1.5 ** 2))
    return g / g.sum()


def taps32():
    return taps64().astype(np.float32)


def window64():
    g = taps64()
    return np.outer(g, g)


# ---- seeded sources ---------------------------------------------------------------------------------------------------------
def picture(seed, N, C, H, W):
    """A smooth picture plus noise on a [0, 1] scale, float64 (N, C, H, W): SSIM of pure noise is 0 whatever the kernel does."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([0.5 + 0.4 * np.sin(xx / 5.0 + c) * np.cos(yy / 4.0 - c) for c in range(C)])
    return np.clip(base[None] + rng.normal(0, 0.08, (N, C, H, W)), 0.0, 1.0)


def as_u8(x):
    """(N, C, H, W) on [0, 1] -> uint8 (N, H, W, C)."""
    return np.ascontiguousarray(np.clip(np.floor(x * 255.0 + 0.5), 0, 255).astype(np.uint8).transpose(0, 2, 3, 1))


def pair(seed, shape, a_u8, b_u8):
    """Two related pictures in the asked forms: b is a with more noise and a small gain, as a restoration beside its truth."""
    N, C, H, W = shape
    a = picture(seed, N, C, H, W)
    rng = np.random.default_rng(seed + 1000)
    b = np.clip(0.97 * a + 0.01 + rng.normal(0, 0.03, a.shape), 0.0, 1.0)
    return (as_u8(a) if a_u8 else a.astype(np.float32)), (as_u8(b) if b_u8 else b.astype(np.float32))


# ---- the pixel pipeline ------------------------------------------------------------------------------------------------------
def _quantize32(v32):
    """min(max(floor(255 v + 0.5), 0), 255) in fp32, as the contract defines it (the rounding of an image about to be saved)."""
    return np.clip(np.floor(v32 * np.float32(255.0) + np.float32(0.5)), np.float32(0.0), np.float32(255.0))


def to255(x, quantize=False):
    """A source in 0..255 units, float64 planar (N, C, H, W)."""
    x = np.asarray(x)
    if x.dtype == np.uint8:
        return x.transpose(0, 3, 1, 2).astype(np.float64)
    assert x.dtype == np.float32
    return _quantize32(x).astype(np.float64) if quantize else x.astype(np.float64) * 255.0


def crop(x, c):
    return x[..., c:x.shape[-2] - c, c:x.shape[-1] - c] if c else x


def luma(x):
    return (16.0 + (65.481 * x[:, 0] + 128.553 * x[:, 1] + 24.966 * x[:, 2]) / 255.0)[:, None]


def prepare(x, crop_border=0, y_channel=False, quantize=False):
    x = crop(to255(x, quantize), crop_border)
    return luma(x) if y_channel else x


# ---- fp64 ----------------------------------------------------------------------------------------------------------------------
def filter_valid(x, g=None):
    """The windowed mean of every plane of x (..., H, W) at the (H - 10) x (W - 10) positions where the window fits."""
    g = taps64() if g is None else g
    H, W = x.shape[-2:]
    h = sum(g[j] * x[..., :, j:j + W - WIN + 1] for j in range(WIN))
    return sum(g[j] * h[..., j:j + H - WIN + 1, :] for j in range(WIN))


def moments(a, b):
    return filter_valid(a), filter_valid(b), filter_valid(a * a), filter_valid(b * b), filter_valid(a * b)


def ssim_map(a, b):
    mu1, mu2, e11, e22, e12 = moments(a, b)
    s1, s2, s12 = e11 - mu1 * mu1, e22 - mu2 * mu2, e12 - mu1 * mu2
    return (2 * mu1 * mu2 + C1) * (2 * s12 + C2) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))


def mse(a, b):
    d = a - b
    return (d * d).reshape(d.shape[0], -1).sum(axis=1) / float(d[0].size)


def ssim(a, b):
    if min(a.shape[-2:]) < WIN:
        raise ValueError("ssim: the cropped image is smaller than the 11 x 11 window")
    return ssim_map(a, b).reshape(a.shape[0], -1).mean(axis=1)


def psnr_from_mse(m):
    return float("inf") if m == 0 else 10.0 * np.log10(255.0 ** 2 / m)


def evaluate(a, b, crop_border=0, y_channel=False, quantize=(False, False)):
    """fp64 (N, 2) = {MSE, SSIM}; SSIM is NaN where the cropped image cannot hold a window."""
    pa = prepare(a, crop_border, y_channel, quantize[0])
    pb = prepare(b, crop_border, y_channel, quantize[1])
    if pa.shape != pb.shape or pa.shape[-1] <= 0 or pa.shape[-2] <= 0:
        raise ValueError("evaluate: shapes differ or nothing is left of them")
    s = ssim(pa, pb) if min(pa.shape[-2:]) >= WIN else np.full(pa.shape[0], np.nan)
    return np.stack([mse(pa, pb), s], axis=1)


# ---- fp32, rounded where the kernel rounds --------------------------------------------------------------------------------------
def _fma32(g, v, acc):
    """fmaf: the product of two fp32 is exact in the 64-bit significand of long double, the sum is rounded there once and once
    more to fp32 (a double rounding can differ from fmaf only when that sum sits within 2^-40 of an fp32 tie)."""
    return (np.longdouble(g) * v.astype(np.longdouble) + acc.astype(np.longdouble)).astype(np.float32)


def _to255_32(x, quantize):
    x = np.asarray(x)
    if x.dtype == np.uint8:
        return x.transpose(0, 3, 1, 2).astype(np.float32)
    return _quantize32(x) if quantize else x * np.float32(255.0)


def _luma32(x):
    f = np.float32
    t = f(65.481) * x[:, 0]
    t = t + f(128.553) * x[:, 1]
    t = t + f(24.966) * x[:, 2]
    return (f(16.0) + t / f(255.0))[:, None]


def _prepare32(x, crop_border, y_channel, quantize):
    x = crop(_to255_32(x, quantize), crop_border)
    return _luma32(x) if y_channel else x


def _chain32(x, axis_len, along_x):
    g = taps32()
    out_len = axis_len - WIN + 1
    acc = np.zeros(x.shape[:-1] + (out_len,) if along_x else x.shape[:-2] + (out_len, x.shape[-1]), dtype=np.float32)
    for j in range(WIN):
        acc = _fma32(g[j], x[..., :, j:j + out_len] if along_x else x[..., j:j + out_len, :], acc)
    return acc


def _filter32(x):
    H, W = x.shape[-2:]
    return _chain32(_chain32(x, W, True), H, False)


def _thread_sums(values, per_thread):
    """values (..., per_thread, NT): every thread's sequential fp32 sum from 0, then fp64."""
    acc = np.zeros(values.shape[:-2] + (values.shape[-1],), dtype=np.float32)
    for k in range(per_thread):
        acc = acc + values[..., k, :]
    return acc.astype(np.float64)


def evaluate32(a, b, crop_border=0, y_channel=False, quantize=(False, False), what=("psnr", "ssim")):
    f = np.float32
    pa = _prepare32(a, crop_border, y_channel, quantize[0])
    pb = _prepare32(b, crop_border, y_channel, quantize[1])
    N, P, H, W = pa.shape
    d = pa - pb
    sq = d * d
    out = np.full((N, 2), np.nan)
    tiled = "ssim" in what
    if not tiled:                                        # the MSE-only launch: plane-major elements, PE per thread, strided by NT
        flat = sq.reshape(N, -1)
        pad = (-flat.shape[1]) % (NT * PE)
        flat = np.concatenate([flat, np.zeros((N, pad), f)], axis=1).reshape(N, -1, PE, NT)
        out[:, 0] = _thread_sums(flat, PE).reshape(N, -1).sum(axis=1) / float(P * H * W)
        return out
    mh, mw = H - WIN + 1, W - WIN + 1
    nty, ntx = -(-mh // TILE), -(-mw // TILE)
    S = TILE + WIN - 1
    total = np.zeros(N)
    for by in range(nty):                                # squared differences: each tile's staged square, STAGE pixels per thread
        for bx in range(ntx):
            stage = np.zeros((N, P, S, S), f)
            y0, x0 = by * TILE, bx * TILE
            part = sq[:, :, y0:y0 + S, x0:x0 + S]
            stage[:, :, :part.shape[2], :part.shape[3]] = part
            if bx != ntx - 1:
                stage[:, :, :, TILE:] = 0
            if by != nty - 1:
                stage[:, :, TILE:, :] = 0
            flat = np.concatenate([stage.reshape(N, P, S * S), np.zeros((N, P, STAGE * NT - S * S), f)], axis=2)
            total += _thread_sums(flat.reshape(N, P, STAGE, NT), STAGE).reshape(N, -1).sum(axis=1)
    if "psnr" in what:
        out[:, 0] = total / float(P * H * W)
    a0, b0 = pa - f(PIVOT), pb - f(PIVOT)
    m0, m1, m2, m3, m4 = _filter32(a0), _filter32(b0), _filter32(a0 * a0), _filter32(b0 * b0), _filter32(a0 * b0)
    s1, s2, s12 = m2 - m0 * m0, m3 - m1 * m1, m4 - m0 * m1
    mu1, mu2 = m0 + f(PIVOT), m1 + f(PIVOT)
    num = (f(2.0) * mu1 * mu2 + f(C1)) * (f(2.0) * s12 + f(C2))
    den = (mu1 * mu1 + mu2 * mu2 + f(C1)) * (s1 + s2 + f(C2))
    v = num / den
    padded = np.zeros((N, P, nty * TILE, ntx * TILE), f)
    padded[:, :, :mh, :mw] = v
    rows = TILE // (NT // TILE)                          # map values per thread: rows tr, tr + 8, tr + 16, tr + 24 of its column
    per = padded.reshape(N, P, nty, rows, NT // TILE, ntx * TILE)
    acc = np.zeros((N, P, nty, NT // TILE, ntx * TILE), f)
    for k in range(rows):
        acc = acc + per[:, :, :, k]
    out[:, 1] = acc.astype(np.float64).reshape(N, -1).sum(axis=1) / float(P * mh * mw)
    return out


# ---- the worst-case bound ------------------------------------------------------------------------------------------------------
def pixel_error(u8_or_quantized, y_channel):
    """|fp32 pixel value - exact pixel value| in 0..255 units: 0 for an 8-bit source, one rounding of 255 v otherwise; Y adds the
    roundings of its three constants, three products, two sums, the division and the final sum (t <= 219 * 255, Y <= 235)."""
    e = 0.0 if u8_or_quantized else 255.0 * U
    return e + (7 * 219.0 + 235.0) * U if y_channel else e


def bounds(a_exact, b_exact, y_channel):
    """(bound on |MSE - fp64 MSE|, bound on |SSIM - fp64 SSIM|) for sources whose pixel values carry pixel_error(...)."""
    ea, eb = pixel_error(a_exact, y_channel), pixel_error(b_exact, y_channel)
    R, A = 255.0, 128.0
    # MSE: d = fl(a - b), fl(d * d), a thread's sum of at most 8 squares (7 additions of a partial sum below 8 * 255^2)
    ed = ea + eb + R * U
    b_mse = 2 * R * ed + ed * ed + R * R * U + 7 * R * R * U + 1e-9
    # staged values about the pivot: the subtraction of 128 is exact for integers
    sa, sb = (ea + (A * U if ea else 0.0)), (eb + (A * U if eb else 0.0))
    passes = 2 * (WIN + 2) * U                           # per axis: 11 fmaf roundings, the taps' own rounding, second order
    e_mu1, e_mu2 = sa + passes * A, sb + passes * A
    e_e11 = 2 * A * sa + sa * sa + A * A * U + passes * A * A
    e_e22 = 2 * A * sb + sb * sb + A * A * U + passes * A * A
    e_e12 = A * (sa + sb) + sa * sb + A * A * U + passes * A * A
    e_s1 = e_e11 + 2 * A * e_mu1 + e_mu1 ** 2 + 2 * A * A * U
    e_s2 = e_e22 + 2 * A * e_mu2 + e_mu2 ** 2 + 2 * A * A * U
    e_s12 = e_e12 + A * (e_mu1 + e_mu2) + e_mu1 * e_mu2 + 2 * A * A * U
    er = max(e_mu1, e_mu2) + R * U                       # the means moved back by 128
    # luminance term (2 r1 r2 + C1) / (r1^2 + r2^2 + C1): (r1 + r2) / (r1^2 + r2^2 + C1) <= 1 / sqrt(2 C1)
    dl = 2 * (2 * er / np.sqrt(2 * C1) + 2 * er * er / C1 + 4 * U)
    # contrast-structure term (2 s12 + C2) / (s1 + s2 + C2) with |term| <= 1 and a denominator of at least C2
    e_n2 = 2 * e_s12 + (2 * A * A + 2 * C2) * U
    e_d2 = e_s1 + e_s2 + (4 * A * A + 2 * C2) * U
    dcs = (e_n2 + e_d2) / (C2 - e_d2)
    # the two products, the division, a thread's sum of 4 map values
    b_ssim = dl + dcs + dl * dcs + 8 * U
    return b_mse, b_ssim
