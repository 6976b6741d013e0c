"""fp64 restatement of the DISTS contract (DESIGN.md section 7 "DISTS"; Ding et al., TPAMI 2020, VGG-16) for the tests: plain
torch.nn.functional on the CPU, no package code.  `storage=` is the rounding model of the device path: weights, biases, the
prepared image, every conv output and every L2-pool output are rounded to fp16 or bf16; `accumulate=` is the type the convs sum
in (torch.float32 as the MFMA does, or torch.float64: another summation order of the same rounded operands).

The bounds of the device kernels against this file, from the rounding points (u = 2^-24 for fp32, U = 2^-53 for fp64):

l2pool, on the same 16-bit inputs.  The nine terms w x^2 are exact in fp32 (a 16-bit value has at most 11 significant bits, its
  square at most 22, the weights are powers of two) and non-negative, so the eight additions cost at most (1 + u)^8 - 1 relative
  on the sum, whatever their order; adding the fp32 constant 1e-12 (itself rounded) is one more factor: t^ = t (1 + e), |e| <= 9 u
  to first order.  The square root halves that and rounds once: 5.5 u.  The store rounds once to the 16-bit type: ROUNDING[dt]
  relative for a normal result, and half the subnormal spacing, TINY[dt], absolute below the smallest normal number (fp16: the
  planted sqrt(1e-12) = 1e-6 is subnormal there).  So  |out - exact| <= 1.001 (5.5 u + ROUNDING[dt]) exact + TINY[dt].
stats.  Every product is exact in fp64 (16-bit operands: 22 bits; fp32 operands of the image: 48 bits), so the error of a sum of
  n terms is the summation's alone: at most (n - 1) U sum |terms| for any order (x 1.001 for the higher orders).  `sums` adds in
  80-bit long double, whose own error, n 2^-64 sum |terms|, is a two-thousandth of that.
scores.  `dists` forms the means, E[a^2] - mu^2 and E[ab] - mu_a mu_b, S1, S2 and the channel sums of its raw-sum form in long
  double as well.  In fp64 that subtraction loses about 2^-53 mu^2, which S2 divides by sigma_a^2 + sigma_b^2 + 1e-6: on a
  stage of two pixels (the fifth of a 16 x 19 image) a texture term then moves by 1e-16 .. 4e-16 with the last bit of the conv
  outputs, that is with the machine's fp64 summation order, and the comparison with the two-pass form (test_dists_cpu.py, 2e-16)
  would measure the host instead of the contract.  `similarities` keeps the fp64 arithmetic, which is the device path's; its
  distance from this reference is far inside every bar of test_dists_gpu.py (1e-12 at stage 0, 3 x e_model >= 7e-7 elsewhere).
"""
import numpy as np
import torch
import torch.nn.functional as F

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
STAGES = ((0, 2), (5, 7), (10, 12, 14), (17, 19, 21), (24, 26, 28))
C1 = C2 = 1e-6
U32 = 2.0 ** -24
U64 = 2.0 ** -53
ROUNDING = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
TINY = {torch.float16: 2.0 ** -25, torch.bfloat16: 0.0}
HANN = (0.25, 0.5, 0.25)                # np.hanning(5)[1:-1], normalised; the 3x3 window is its outer product


def rounded(t, storage):
    """t (fp64 or fp32) as the device stores it: through fp32 to `storage`, back as fp64; unchanged without a storage type."""
    return t if storage is None else t.float().to(storage).double()


def prep(x01, mean=MEAN, std=STD, storage=None):
    """(N, 3, H, W) on a [0, 1] scale -> (x - mean) / std, fp64."""
    m = torch.tensor(mean, dtype=torch.float64).view(1, 3, 1, 1)
    s = torch.tensor(std, dtype=torch.float64).view(1, 3, 1, 1)
    return rounded((x01.double() - m) / s, storage)


def conv(x, w, b, storage=None, accumulate=torch.float32):
    """3x3, pad 1, bias; fp64, or `accumulate` sums of `storage`-rounded operands with the result rounded to `storage`."""
    if storage is None:
        return F.conv2d(x, w.double(), b.double(), padding=1)
    return rounded(F.conv2d(x.to(accumulate), rounded(w, storage).to(accumulate), rounded(b, storage).to(accumulate), padding=1), storage)


def l2pool(x):
    """(N, C, H, W) fp64 -> sqrt(sum_{di, dj} g[di] g[dj] x(2i + di, 2j + dj)^2 + 1e-12), zero padding, (N, C, ceil(H/2), ceil(W/2))."""
    N, C, H, W = x.shape
    oh, ow = (H + 1) // 2, (W + 1) // 2
    p = F.pad(x.double().pow(2), (1, 2, 1, 2))                        # index 2i + di + 1 of the padded square
    acc = torch.zeros(N, C, oh, ow, dtype=torch.float64)
    for di in range(3):
        for dj in range(3):
            acc = acc + HANN[di] * HANN[dj] * p[:, :, di:di + 2 * oh:2, dj:dj + 2 * ow:2]
    return (acc + 1e-12).sqrt()


def l2pool_bound(exact, dt):
    return 1.001 * (5.5 * U32 + ROUNDING[dt]) * exact + TINY[dt]


def sums(a, b):
    """(N, C, H, W) each -> long double (N, C, 5) = {sum a, sum b, sum a^2, sum b^2, sum ab} over the pixels, and the same of the
    absolute terms (a, b >= 0 after the ReLU, so it differs only for a signed input)."""
    la, lb = (t.double().numpy().astype(np.longdouble).reshape(t.shape[0], t.shape[1], -1) for t in (a, b))
    terms = (la, lb, la * la, lb * lb, la * lb)
    return np.stack([t.sum(axis=2) for t in terms], axis=2), np.stack([np.abs(t).sum(axis=2) for t in terms], axis=2)


def sums_bound(abs_sums, n):
    return 1.001 * (n - 1) * U64 * abs_sums


def _similarities(s, n):
    mu_a, mu_b = s[..., 0] / n, s[..., 1] / n
    var_a, var_b, cov = s[..., 2] / n - mu_a * mu_a, s[..., 3] / n - mu_b * mu_b, s[..., 4] / n - mu_a * mu_b
    return (2 * mu_a * mu_b + C1) / (mu_a * mu_a + mu_b * mu_b + C1), (2 * cov + C2) / (var_a + var_b + C2)


def similarities(s, n):
    """fp64 (..., 5) raw sums over n pixels -> (S1, S2) of the contract in fp64: the arithmetic of the device path."""
    return _similarities(torch.as_tensor(np.asarray(s, dtype=np.float64)) if not torch.is_tensor(s) else s.double(), n)


def similarities_two_pass(a, b):
    """(S1, S2) of (N, C, H, W) features with the variances and the covariance about the means (the form of the DISTS paper)."""
    a, b = a.double(), b.double()
    mu_a, mu_b = a.mean(dim=(2, 3), keepdim=True), b.mean(dim=(2, 3), keepdim=True)
    var_a, var_b = ((a - mu_a) ** 2).mean(dim=(2, 3)), ((b - mu_b) ** 2).mean(dim=(2, 3))
    cov = ((a - mu_a) * (b - mu_b)).mean(dim=(2, 3))
    mu_a, mu_b = mu_a[:, :, 0, 0], mu_b[:, :, 0, 0]
    return (2 * mu_a * mu_b + C1) / (mu_a * mu_a + mu_b * mu_b + C1), (2 * cov + C2) / (var_a + var_b + C2)


def features(x01, convs, mean=MEAN, std=STD, storage=None, accumulate=torch.float32):
    """The six features of (N, 3, H, W) images, after the ReLU: [x, stage 1, ..., stage 5], fp64."""
    feats, x, j = [x01.float().double()], prep(x01.float(), mean, std, storage), 0
    for k, idx in enumerate(STAGES):
        if k:
            x = rounded(l2pool(x), storage)
        for _ in idx:
            w, b = convs[j]
            x, j = conv(x, w, b, storage, accumulate).clamp_min(0.0), j + 1
        feats.append(x)
    return feats


def dists(a01, b01, convs, alpha, beta, mean=MEAN, std=STD, storage=None, accumulate=torch.float32, two_pass=False):
    """-> (score (N,), terms (N, 6, 2)) fp64: per stage the structure term sum_c alpha_c S1_c / ws and the texture term
    sum_c beta_c S2_c / ws with ws = sum alpha + sum beta; score = 1 - terms.sum()."""
    alpha, beta = (t.double().reshape(-1).numpy().astype(np.longdouble) for t in (alpha, beta))
    ws = alpha.sum() + beta.sum()
    fa, fb = features(a01, convs, mean, std, storage, accumulate), features(b01, convs, mean, std, storage, accumulate)
    terms, at = [], 0
    for xa, xb in zip(fa, fb):
        c, n = xa.shape[1], xa.shape[2] * xa.shape[3]
        if two_pass:
            s1, s2 = similarities_two_pass(xa, xb)
        else:
            s1, s2 = _similarities(sums(xa, xb)[0], np.longdouble(n))          # long double from the long-double sums (see above)
        pair = [(w[at:at + c] * (s.numpy() if torch.is_tensor(s) else s).astype(np.longdouble)).sum(axis=1) / ws
                for w, s in ((alpha, s1), (beta, s2))]
        terms.append(torch.from_numpy(np.stack(pair, axis=1).astype(np.float64)))
        at += c
    terms = torch.stack(terms, dim=1)
    return 1.0 - terms.sum(dim=(1, 2)), terms
