"""Torch restatement of the colour-fix contract (DESIGN.md section 7 "Colour fix"; the definitions StableSR's
`wavelet_color_fix` / `adain_color_fix` made standard).  Plain helper for tests/test_colorfix_*.py; runs in the dtype of its
inputs (fp64 is the reference the kernels are held to, fp32 gives the restatement's own rounding error)."""
import torch
import torch.nn.functional as F

LEVELS = (1, 2, 4, 8, 16)
SIZES = [(5, 7), (8, 8), (24, 40), (257, 131), (768, 1024), (1024, 1024), (2048, 2048)]


def blur(x, r):
    """replicate-pad by r, depthwise 3x3 [[1,2,1],[2,4,2],[1,2,1]] / 16 at dilation r.  (F.pad's replicate mode needs the pad
    below the side length, so the padding is written as the index clamp it is.)"""
    B, C, H, W = x.shape
    ih = torch.arange(-r, H + r).clamp(0, H - 1)
    iw = torch.arange(-r, W + r).clamp(0, W - 1)
    xp = x[:, :, ih][:, :, :, iw]
    k = torch.tensor([[1.0, 2.0, 1.0], [2.0, 4.0, 2.0], [1.0, 2.0, 1.0]], dtype=x.dtype) / 16
    return F.conv2d(xp, k.expand(C, 1, 3, 3).contiguous(), dilation=r, groups=C)


def decompose(x):
    high = torch.zeros_like(x)
    for r in LEVELS:
        low = blur(x, r)
        high = high + (x - low)
        x = low
    return high, x


def wavelet(content, style):
    """The textbook form: high frequencies of the content plus low frequencies of the style."""
    return (decompose(content)[0] + decompose(style)[1]).clamp(0, 1)


def _tap(d, r, dim):
    n = d.shape[dim]
    i = torch.arange(n)
    lo, hi = (i - r).clamp(0, n - 1), (i + r).clamp(0, n - 1)
    return (0.25 * d.index_select(dim, lo) + 0.25 * d.index_select(dim, hi)) + 0.5 * d


def wavelet_difference(content, style):
    """The form the kernel uses: clamp(content + B(style - content)), B separable: five horizontal 3-tap levels, then five
    vertical ones, every index clamped per level."""
    d = style - content
    for r in LEVELS:
        d = _tap(d, r, 3)
    for r in LEVELS:
        d = _tap(d, r, 2)
    return (content + d).clamp(0, 1)


def adain(content, style, eps=1e-5):
    B, C, H, W = content.shape
    if H * W < 2:
        raise ValueError("adain needs at least 2 pixels per plane")

    def stats(x):
        f = x.reshape(B, C, -1)
        return f.mean(2).view(B, C, 1, 1), (f.var(2, unbiased=True) + eps).sqrt().view(B, C, 1, 1)

    mc, sc = stats(content)
    ms, ss = stats(style)
    return ((content - mc) / sc * ss + ms).clamp(0, 1)


def apply(content, style, mode):
    return {"wavelet": wavelet, "adain": adain}[mode](content, style)


def recipe(B, H, W, seed, noise=0.05):
    """The seeded inputs of the GPU tests: content = rand, style = clamp(0.7 * avgpool5(content) + 0.2 * rand(B,3,1,1) +
    noise * rand): a blurred, colour-shifted, lightly noised copy, fp32 in [0, 1]."""
    g = torch.Generator().manual_seed(seed)
    content = torch.rand(B, 3, H, W, generator=g)
    pooled = F.avg_pool2d(content, 5, stride=1, padding=2, count_include_pad=False)
    style = (0.7 * pooled + 0.2 * torch.rand(B, 3, 1, 1, generator=g) + noise * torch.rand(B, 3, H, W, generator=g)).clamp(0, 1)
    return content, style


def saturated_fraction(x):
    return ((x == 0) | (x == 1)).float().mean().item()
