"""fp64 restatement of the LPIPS contract (DESIGN.md section 7 "LPIPS"; LPIPS v0.1, net = vgg) for the tests: plain
torch.nn.functional on the CPU, no package code.  `storage=` is the rounding model of the device path: weights, biases, the
prepared image and every conv output are rounded to fp16 or bf16, and each conv accumulates in fp32.
"""
import torch
import torch.nn.functional as F

SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
SLICES = ((0, 2), (5, 7), (10, 12, 14), (17, 19, 21), (24, 26, 28))
U32 = 2.0 ** -24                       # fp32 unit roundoff
ROUNDING = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}


def rounded(t, storage):
    """t (fp64 or fp32) as the device stores it: through fp32 to `storage`, back as fp64; unchanged without a storage type."""
    return t if storage is None else t.float().to(storage).double()


def prep(x01, shift=SHIFT, scale=SCALE, storage=None):
    """(N, 3, H, W) on a [0, 1] scale -> the scaling layer's output, fp64."""
    x = x01.double()
    sh = torch.tensor(shift, dtype=torch.float64).view(1, 3, 1, 1)
    sc = torch.tensor(scale, dtype=torch.float64).view(1, 3, 1, 1)
    return rounded(((2.0 * x - 1.0) - sh) / sc, storage)


def conv(x, w, b, storage=None):
    """3x3, pad 1, bias; fp64, or fp32 accumulation of `storage`-rounded operands with the result rounded to `storage`."""
    if storage is None:
        return F.conv2d(x, w.double(), b.double(), padding=1)
    return rounded(F.conv2d(x.float(), rounded(w, storage).float(), rounded(b, storage).float(), padding=1), storage)


def unit(x):
    return x / (x.pow(2).sum(dim=1, keepdim=True).sqrt() + 1e-10)


def tap(pre_a, pre_b, lin):
    """One tap from the conv's pre-activations (N, C, H, W), fp64: (d map (N, H, W), D (N,), pooled a, pooled b)."""
    a, b = pre_a.double().clamp_min(0.0), pre_b.double().clamp_min(0.0)
    d = ((unit(a) - unit(b)).pow(2) * lin.double().view(1, -1, 1, 1)).sum(dim=1)
    pool = lambda t: F.max_pool2d(t, 2) if min(t.shape[2:]) >= 2 else None
    return d, d.mean(dim=(1, 2)), pool(a), pool(b)


def lpips(a01, b01, convs, lins, shift=SHIFT, scale=SCALE, storage=None):
    """-> (D (N, 5) fp64: the five taps' terms, whose row sum is LPIPS; the five d maps (N, H_l, W_l))."""
    xa, xb = prep(a01, shift, scale, storage), prep(b01, shift, scale, storage)
    D, maps, j = [], [], 0
    for l, idx in enumerate(SLICES):
        for i in idx:
            w, b = convs[j]
            xa, xb, j = conv(xa, w, b, storage), conv(xb, w, b, storage), j + 1
            if i != idx[-1]:
                xa, xb = xa.clamp_min(0.0), xb.clamp_min(0.0)
        d, Dl, xa, xb = tap(xa, xb, lins[l])
        D.append(Dl)
        maps.append(d)
    return torch.stack(D, dim=1), maps


def tap_bounds(C, max_w):
    """Bounds of the device tap's fp32 arithmetic against `tap` on the same 16-bit inputs, u = 2^-24, g = C u (first order, x 1.001):
    the channel sum of squares (any order, products fused) carries at most g relative, so 1 / (sqrt + 1e-10) at most g / 2 + 3 u
    (sqrt, add, reciprocal) and a unit feature, |xh_c| <= 1, at most eta = g / 2 + 4 u absolute times |xh_c|; a difference
    e_c = xh_c - yh_c then eta (|xh_c| + |yh_c|) + u |e_c|, its square twice |e_c| times that plus u e_c^2, and the weighted sum g
    more on sum_c w_c e_c^2.  With sum_c (|xh_c| + |yh_c|)^2 <= 4 and sum_c e_c^2 <= 4:
        |err d(p)| <= max_w (8 eta + 12 u + 4 g) = max_w u (8 C + 44)
    D adds the fp32 sum of a quad's four d (3 u of at most 4 max_w each) and an fp64 mean: |err D| <= max_w u (8 C + 56)."""
    return 1.001 * max_w * U32 * (8 * C + 44), 1.001 * max_w * U32 * (8 * C + 56)
