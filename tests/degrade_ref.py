"""The three degradation launches restated for the tests, independent of the product's arithmetic (nothing here imports
instantir_amd); numpy throughout, images (N, C, H, W).

  filter2d64 / filter2d32        k x k correlation with reflect padding; fp64, and fp32 with fmaf in (i, j) order
  filter2d_bound                 (k^2 + 1) 2^-24 sum|taps| max|in|;  filter2d_bound32: one fp32 ulp of that magnitude
  philox4x32_10                  the generator (Random123), vectorised
  normal64 / noise64 / noise32   z from the contract's fp32 uniforms, then fp64 (or numpy-fp32) log / sqrt / cos
  noise_bound                    the element-wise bound of the noise launch for a given ulp budget of z
  jpeg64 / jpeg32                the 4:2:0 round trip in fp64 (with each block's tie distances and the element-wise error
                                 bound of an fp32 evaluation), and in fp32 with the kernel's rounding points
  smooth_noise_image             the seeded smooth-plus-noise 8-bit images of the JPEG tests
"""
import numpy as np

U = 2.0 ** -24                      # unit roundoff of fp32: one rounding of a value v errs by at most U |v|


def _fmaf(a, b, c):
    """round32(a * b + c): the product of two fp32 values is exact in fp64; the sum is rounded to fp64 and then to fp32"""
    return (np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
            + np.asarray(c, np.float32).astype(np.float64)).astype(np.float32)


# ---- filter2d ---------------------------------------------------------------------------------------------------------------
def _reflect_index(n, r):
    t = np.arange(-r, n + r)
    t = np.where(t < 0, -t, t)
    return np.where(t >= n, 2 * (n - 1) - t, t)


def _padded(x, r):
    H, W = x.shape[-2:]
    return x[..., _reflect_index(H, r), :][..., _reflect_index(W, r)]


def filter2d64(x, taps):
    """x (N, C, H, W), taps (N, k, k) -> fp64"""
    x, taps = np.asarray(x, np.float64), np.asarray(taps, np.float64)
    k = taps.shape[-1]
    H, W = x.shape[-2:]
    p = _padded(x, (k - 1) // 2)
    out = np.zeros_like(x)
    for i in range(k):
        for j in range(k):
            out += taps[:, None, i, j, None, None] * p[..., i:i + H, j:j + W]
    return out


def filter2d32(x, taps):
    """the kernel's arithmetic: acc = fmaf(tap[i][j], pixel, acc) from 0, i outer, j inner"""
    x, taps = np.asarray(x, np.float32), np.asarray(taps, np.float32)
    k = taps.shape[-1]
    H, W = x.shape[-2:]
    p = _padded(x, (k - 1) // 2)
    acc = np.zeros_like(x)
    for i in range(k):
        for j in range(k):
            acc = _fmaf(np.broadcast_to(taps[:, None, i, j, None, None], x.shape), p[..., i:i + H, j:j + W], acc)
    return acc


def filter2d_bound(x, taps):
    """Per image: every one of the k^2 fmaf rounds a partial sum of magnitude <= S = sum|taps| max|in| (to first order; the +1
    covers the second-order growth of the partial sums themselves, k^2 U S << S), so |error| <= (k^2 + 1) U S.  The fp64
    restatement runs on the same fp32 taps and pixels: nothing else is rounded.  -> (N, 1, 1, 1)"""
    x, taps = np.asarray(x, np.float64), np.asarray(taps, np.float64)
    k = taps.shape[-1]
    S = np.abs(taps).sum(axis=(1, 2)) * np.abs(x).max(axis=(1, 2, 3))
    return ((k * k + 1) * U * S)[:, None, None, None]


def filter2d_bound32(x, taps):
    """against filter2d32, which rounds where the kernel rounds: the restatement's fmaf (fp64 sum, then fp32) can land one
    fp32 ulp beside the fused result; one ulp of a value of magnitude S"""
    x, taps = np.asarray(x, np.float64), np.asarray(taps, np.float64)
    S = np.abs(taps).sum(axis=(1, 2)) * np.abs(x).max(axis=(1, 2, 3))
    return (2.0 * U * S)[:, None, None, None]


# ---- Philox and the normal transform ----------------------------------------------------------------------------------------
PHILOX_KNOWN = (
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (broadcastable), key: two uint32 scalars -> four uint32 arrays"""
    M = 0xffffffff
    c = [np.asarray(v, np.uint64) & M for v in np.broadcast_arrays(*counter)]
    k0, k1 = int(key[0]) & M, int(key[1]) & M
    for _ in range(10):
        p0, p1 = c[0] * np.uint64(0xD2511F53), c[2] * np.uint64(0xCD9E8D57)
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & M, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & M]
        k0, k1 = (k0 + 0x9E3779B9) & M, (k1 + 0xBB67AE85) & M
    return [v.astype(np.uint32) for v in c]


def uniforms32(r):
    """((float)(r >> 8) + 0.5f) * 2^-24 in fp32: exact below 2^23, rounded to even above, in (0, 1]"""
    return ((r >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)


def _uniform_pair(shape, seed, stream, gray):
    N, C, H, W = shape
    n, c, y, x = np.meshgrid(np.arange(N), np.arange(C), np.arange(H), np.arange(W), indexing="ij")
    r = philox4x32_10((y * W + x, n, np.zeros_like(c) if gray else c, np.full_like(c, stream)), (seed & 0xffffffff, seed >> 32))
    return uniforms32(r[0]), uniforms32(r[1])


def normal64(shape, seed, stream=0, gray=False):
    u1, u2 = _uniform_pair(shape, seed, stream, gray)
    return np.sqrt(-2.0 * np.log(u1.astype(np.float64))) * np.cos(2.0 * np.pi * u2.astype(np.float64))


def noise64(x, sigma, seed, stream=0, gray=False):
    """-> (clamped result, unclamped result), fp64; sigma: one fp32 value per image"""
    x = np.asarray(x, np.float64)
    s = np.asarray(sigma, np.float32).astype(np.float64).reshape(-1, 1, 1, 1) / 255.0
    raw = x + s * normal64(x.shape, seed, stream, gray)
    return np.clip(raw, 0.0, 1.0), raw


def noise32(x, sigma, seed, stream=0, gray=False):
    """fp32 at the kernel's rounding points; log and sqrt are numpy's fp32 ones, cospif is the fp64 cosine rounded to fp32 (the
    argument 2 u2 is exact; pi * (2 u2) rounded to fp32 would not be) -- not the device's functions"""
    x = np.asarray(x, np.float32)
    u1, u2 = _uniform_pair(x.shape, seed, stream, gray)
    z = np.sqrt(np.float32(-2.0) * np.log(u1)) * np.cos(np.pi * 2.0 * u2.astype(np.float64)).astype(np.float32)
    s = (np.asarray(sigma, np.float32) / np.float32(255.0)).reshape(-1, 1, 1, 1)
    return np.clip(x + s * z, np.float32(0.0), np.float32(1.0)).astype(np.float32)


Z_MAX = 5.9                        # sqrt(-2 ln(2^-25)) = 5.887...
NOISE_Z_ULPS = 3.3                 # the budget of z = sqrtf(-2 logf(u1)) * cospif(2 u2) against fp64, in units of 2^-23 |z|:
                                   # twice the 1.611 measured on an MI355X over the 32652 positive samples of test_degrade_gpu.py


def noise_bound(x, sigma, z_ulps):
    """|z - z64| <= z_ulps 2^-23 Z_MAX (the budget of logf, sqrtf, cospif and their product); then sigma / 255, its product with z
    and the sum with x are one rounding each: with s = sigma / 255, |error| <= s Z_MAX (z_ulps 2^-23 + 2 U) + U (|x| + s Z_MAX)."""
    s = np.asarray(sigma, np.float64).reshape(-1, 1, 1, 1) / 255.0
    return s * Z_MAX * (z_ulps * 2.0 * U + 2.0 * U) + U * (np.abs(np.asarray(x, np.float64)) + s * Z_MAX)


# ---- JPEG -------------------------------------------------------------------------------------------------------------------
T_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51,
                   87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120,
                   101, 72, 92, 95, 98, 112, 100, 103, 99], np.float64).reshape(8, 8)
T_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99,
                     99, 99, 99, 99] + [99] * 32, np.float64).reshape(8, 8)
_u, _k = np.arange(8)[:, None], np.arange(8)[None, :]
DCT = np.where(_u == 0, np.sqrt(1.0 / 8.0), 0.5) * np.cos((2 * _k + 1) * _u * np.pi / 16.0)      # D[u][k], fp64
DCT32 = DCT.astype(np.float32)

# The error of an fp32 evaluation (derivation in DESIGN.md section 7 "Synthetic degradation"), in 0..255 units:
#   a block's input sample: 255 v (1 rounding), the colour row (3 or 4 operations on values <= 255, the fp32 coefficients, the
#   inherited input error), the 2 x 2 mean (three sums), the - 128: at most 8.5 roundings of 255.
#   a forward coefficient: each pass multiplies an inherited error by at most A = max_u sum_k |D[u][k]| = 2 sqrt(2) and adds 9 U
#   (8 fmaf and the fp32 basis) times its own magnitude bound, 128 A then 128 A^2 = 1024.
E_IN = 8.5 * 255.0 * U
E_COEF = 8.0 * E_IN + 18.0 * 1024.0 * U


def quality_factor(q):
    q = np.clip(np.asarray(q, np.float64), 1.0, 99.0)
    return np.where(q < 50.0, 5000.0 / q, 200.0 - 2.0 * q) / 100.0


def _blocks(p):
    """(N, H, W) with H, W multiples of 8 -> (N, H/8, W/8, 8, 8)"""
    N, H, W = p.shape
    return p.reshape(N, H // 8, 8, W // 8, 8).transpose(0, 1, 3, 2, 4)


def _unblocks(b):
    N, by, bx = b.shape[:3]
    return b.transpose(0, 1, 3, 2, 4).reshape(N, by * 8, bx * 8)


def _pad16(x):
    H, W = x.shape[-2:]
    return np.pad(x, ((0, 0), (0, 0), (0, -H % 16), (0, -W % 16)), mode="edge")


def jpeg64(x, quality):
    """x (N, 3, H, W) fp32 / fp64 in [0, 1], quality one fp32 value per image -> dict:
      out      fp64 (N, 3, H, W)
      err      element-wise bound on what an fp32 evaluation with no rounding flip may differ by, [0, 1] units
      tie_y    (N, H16/8, W16/8): over each luma block, min over coefficients of (distance of c / step to the nearest tie - tau)
      tie_c    (N, H16/16, W16/16): the same over the Cb and Cr block of each MCU;  negative = a flip cannot be excluded
    tau = E_COEF / step + 4 U |c / step| (three roundings in the fp32 step, one in the division)."""
    x = np.asarray(x, np.float64)
    N, _, H, W = x.shape
    f = quality_factor(np.asarray(quality, np.float32)).reshape(N, 1, 1, 1, 1)
    p = _pad16(255.0 * np.clip(x, 0.0, 1.0))
    R, G, B = p[:, 0], p[:, 1], p[:, 2]
    Y = 0.299 * R + 0.587 * G + 0.114 * B
    Cb = -0.168736 * R - 0.331264 * G + 0.5 * B + 128.0
    Cr = 0.5 * R - 0.418688 * G - 0.081312 * B + 128.0
    mean = lambda c: 0.25 * (c[:, 0::2, 0::2] + c[:, 0::2, 1::2] + c[:, 1::2, 0::2] + c[:, 1::2, 1::2])
    absD = np.abs(DCT)

    def roundtrip(plane, T):
        X = _blocks(plane - 128.0)
        c = DCT @ X @ DCT.T
        step = T * f
        ratio = c / step
        tau = E_COEF / step + 4.0 * U * np.abs(ratio)
        tie = (np.abs(ratio - np.floor(ratio) - 0.5) - tau).min(axis=(-1, -2))
        cq = np.rint(ratio) * step
        Xq = DCT.T @ cq @ DCT
        # the inverse in fp32: c' carries the step's three roundings and its own; each pass multiplies an inherited error by
        # |D| and adds 9 U times the magnitudes it sums
        e_c = 4.0 * U * np.abs(cq)
        mag_s = np.abs(cq) @ absD
        e_s = e_c @ absD + 9.0 * U * mag_s
        e_x = absD.T @ e_s + 9.0 * U * (absD.T @ mag_s)
        return _unblocks(Xq) + 128.0, _unblocks(e_x) + U * (np.abs(_unblocks(Xq)) + 128.0), tie

    Yq, eY, tie_y = roundtrip(Y, T_LUMA)
    Cbq, eB, tie_b = roundtrip(mean(Cb), T_CHROMA)
    Crq, eR, tie_r = roundtrip(mean(Cr), T_CHROMA)
    up = lambda c: np.repeat(np.repeat(c, 2, axis=1), 2, axis=2)
    db, dr, eB, eR = up(Cbq) - 128.0, up(Crq) - 128.0, up(eB), up(eR)
    rgb = np.stack([Yq + 1.402 * dr, Yq - 0.344136 * db - 0.714136 * dr, Yq + 1.772 * db], axis=1)
    # the colour rows: inherited errors through |coefficients|, and per row at most 8 roundings (operations, fp32 coefficients,
    # the - 128) of the magnitudes involved
    mag = np.abs(Yq) + 2.0 * np.abs(db) + 2.0 * np.abs(dr) + 128.0
    e_rgb = np.stack([eY + 1.402 * eR, eY + 0.344136 * eB + 0.714136 * eR, eY + 1.772 * eB], axis=1) + 8.0 * U * mag[:, None]
    out = np.clip(rgb, 0.0, 255.0) / 255.0
    return {"out": out[:, :, :H, :W], "err": (e_rgb / 255.0 + 2.0 * U)[:, :, :H, :W], "tie_y": tie_y, "tie_c": np.minimum(tie_b, tie_r)}


def jpeg_keep_mask(res, H, W):
    """(N, H, W) bool: pixels whose luma block and whose MCU's chroma blocks are all clear of a tie; and the share of 8 x 8
    luma-block positions left out, per image"""
    ok_c = np.repeat(np.repeat(res["tie_c"] > 0, 2, axis=1), 2, axis=2)
    ok = (res["tie_y"] > 0) & ok_c
    share = 1.0 - ok.reshape(ok.shape[0], -1).mean(axis=1)
    return np.repeat(np.repeat(ok, 8, axis=1), 8, axis=2)[:, :H, :W], share


def _dct_pass32(Dm, X, axis):
    """out[..., v] = sum_k Dm[v][k] X[..., k] along `axis` (-1 or -2), fmaf from 0 in k order"""
    X = np.moveaxis(X, axis, -1)
    acc = np.zeros(X.shape, np.float32)
    for k in range(8):
        acc = _fmaf(np.broadcast_to(Dm[:, k], X.shape), np.broadcast_to(X[..., k:k + 1], X.shape), acc)
    return np.moveaxis(acc, -1, axis)


def jpeg32(x, quality):
    """The kernel's arithmetic in numpy fp32 (include/instantir_hip.h: iir_jpeg_roundtrip_f32)."""
    f32 = np.float32
    x = np.asarray(x, f32)
    N, _, H, W = x.shape
    q = np.clip(np.asarray(quality, f32), f32(1), f32(99)).reshape(N, 1, 1, 1, 1)
    with np.errstate(all="ignore"):
        f = (np.where(q < f32(50), f32(5000) / q, f32(200) - f32(2) * q) / f32(100)).astype(f32)
    p = _pad16(f32(255) * np.clip(x, f32(0), f32(1)))
    R, G, B = p[:, 0], p[:, 1], p[:, 2]
    c = lambda v: np.broadcast_to(f32(v), R.shape)
    Y = _fmaf(c(0.114), B, _fmaf(c(0.587), G, f32(0.299) * R))
    Cb = _fmaf(c(0.5), B, _fmaf(c(-0.331264), G, f32(-0.168736) * R)) + f32(128)
    Cr = _fmaf(c(-0.081312), B, _fmaf(c(-0.418688), G, f32(0.5) * R)) + f32(128)
    mean = lambda v: ((v[:, 0::2, 0::2] + v[:, 0::2, 1::2]) + (v[:, 1::2, 0::2] + v[:, 1::2, 1::2])) * f32(0.25)

    def roundtrip(plane, T):
        X = _blocks(plane - f32(128))
        t = _dct_pass32(DCT32, X, -1)
        cf = _dct_pass32(DCT32, t, -2)
        step = (T.astype(f32) * f).astype(f32)
        cq = (np.rint(cf / step) * step).astype(f32)
        s = _dct_pass32(DCT32.T.copy(), cq, -1)
        Xq = _dct_pass32(DCT32.T.copy(), s, -2)
        return _unblocks(Xq) + f32(128)

    Yq = roundtrip(Y, T_LUMA)
    up = lambda v: np.repeat(np.repeat(v, 2, axis=1), 2, axis=2)
    db, dr = up(roundtrip(mean(Cb), T_CHROMA)) - f32(128), up(roundtrip(mean(Cr), T_CHROMA)) - f32(128)
    rgb = np.stack([_fmaf(c(1.402), dr, Yq), _fmaf(c(-0.714136), dr, _fmaf(c(-0.344136), db, Yq)), _fmaf(c(1.772), db, Yq)], axis=1)
    return (np.clip(rgb, f32(0), f32(255)) / f32(255)).astype(f32)[:, :, :H, :W]


def smooth_noise_image(shape, seed, gray_noise=2, channel_noise=6, chroma=0.1):
    """(N, 3, H, W) uint8: low-frequency waves shared by the channels, a tenth of that again per channel, uniform integer
    noise of +-gray_noise levels per pixel and of +-channel_noise levels per element"""
    N, C, H, W = shape
    g = np.random.Generator(np.random.Philox(key=seed))
    y, x = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")

    def wave():
        a, b, ph = g.uniform(0.5, 3.0, 2), g.uniform(0.5, 3.0, 2), g.uniform(0, 2 * np.pi, 2)
        return 50 * np.sin(2 * np.pi * (a[0] * x + b[0] * y) + ph[0]) + 40 * np.cos(2 * np.pi * (a[1] * x - b[1] * y) + ph[1])

    img = np.empty(shape)
    for n in range(N):
        base, gn = wave(), g.integers(-gray_noise, gray_noise + 1, size=(H, W))
        for ch in range(C):
            img[n, ch] = 128 + base + chroma * wave() + gn + g.integers(-channel_noise, channel_noise + 1, size=(H, W))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def exact_jpeg_input(shape, quality, seed):
    """(N, 3, H, W) fp32 in [0.05, 0.95] (H, W multiples of 16) none of whose coefficients is near a rounding tie: integer
    levels qc and offsets delta in [-0.35, 0.35] per coefficient, (qc + delta) T f inverse-transformed in fp64, chroma constant
    over each 2 x 2, converted to RGB, rounded to fp32.  The ranges the levels are drawn from shrink until every value lies inside [0.05, 0.95]
    (the levels stay integers: scaling the finished image would move the ratios)."""
    N, _, H, W = shape
    f = quality_factor(np.asarray(quality, np.float32)).reshape(N, 1, 1, 1, 1)
    up = lambda c: np.repeat(np.repeat(c, 2, axis=1), 2, axis=2)
    for shrink in (1.0, 0.7, 0.5, 0.35, 0.25):
        g = np.random.Generator(np.random.Philox(key=seed))

        def plane(h, w, T, dc_range, ac_range):
            step = T * f
            qc = np.rint(g.uniform(-1, 1, (N, h // 8, w // 8, 8, 8)) * np.floor(shrink * ac_range / step))
            qc[..., 0, 0] = np.rint(g.uniform(-1, 1, (N, h // 8, w // 8)) * np.floor(shrink * dc_range / step[..., 0, 0]))
            delta = g.uniform(-0.35, 0.35, qc.shape) * np.minimum(1.0, 8.0 * shrink / step)     # (a coarse step: a smaller offset)
            return _unblocks(DCT.T @ ((qc + delta) * step) @ DCT) + 128.0

        Y = plane(H, W, T_LUMA, 320.0, 24.0)                      # coefficient ranges in 0..255 units: DC 320 = 40 levels
        db, dr = up(plane(H // 2, W // 2, T_CHROMA, 160.0, 16.0)) - 128.0, up(plane(H // 2, W // 2, T_CHROMA, 160.0, 16.0)) - 128.0
        rgb = np.stack([Y + 1.402 * dr, Y - 0.344136 * db - 0.714136 * dr, Y + 1.772 * db], axis=1) / 255.0
        if rgb.min() >= 0.05 and rgb.max() <= 0.95:
            return rgb.astype(np.float32)
    raise AssertionError("no amplitude keeps the image inside [0.05, 0.95]")
