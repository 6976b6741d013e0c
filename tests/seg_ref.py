"""fp64 restatement of smoothed-energy guidance's query blur (SEG; Hong 2024), independent of instantir_amd.seg: kernel length,
taps, reflect index, the separable blur, the mean mode -- and a helper that gives the CPU oracle's self-attention the SEG form
for the perturbed rows of selected layers without editing oracle/."""
import math

import torch

MEAN_ABOVE = 9999.0


def kernel_length(sigma, n):
    """k0 = ceil(6 sigma) + 1 - (ceil(6 sigma) mod 2); k = min(k0, n + 1) for even n, min(k0, n) for odd n; n = 1 -> 1."""
    cap = 1 if n == 1 else (n + 1 if n % 2 == 0 else n)
    if math.isinf(sigma):
        return cap
    c = math.ceil(6.0 * sigma)
    return min(c + 1 - c % 2, cap)


def weights(sigma, n):
    """(k,) fp64: w_i ~ exp(-(x_i / sigma)^2 / 2), x_i = i - (k - 1) / 2, summing to 1."""
    k = kernel_length(sigma, n)
    x = torch.arange(k, dtype=torch.float64) - (k - 1) / 2.0
    w = torch.exp(-0.5 * (x / sigma) ** 2)
    return w / w.sum()


def reflect_index(i, n):
    """Reflect without repeating the edge: -i -> i, n - 1 + i -> n - 1 - i (|overhang| <= n - 1)."""
    if i < 0:
        i = -i
    if i > n - 1:
        i = 2 * (n - 1) - i
    assert 0 <= i < n
    return i


def _axis(q, w, dim):
    n, k = q.shape[dim], len(w)
    out = torch.zeros_like(q)
    for j in range(k):
        idx = torch.tensor([reflect_index(p + j - k // 2, n) for p in range(n)])
        out = out + w[j] * q.index_select(dim, idx)
    return out


def blur(q, sigma):
    """q (images, H, W, C) -> G_y * G_x * q in fp64, each channel on its own."""
    q = q.double()
    return _axis(_axis(q, weights(sigma, q.shape[2]), 2), weights(sigma, q.shape[1]), 1)


def mean_q(q):
    q = q.double()
    return q.mean(dim=(1, 2), keepdim=True).expand_as(q).clone()


def is_mean(sigma):
    return sigma > MEAN_ABOVE


def seg_q(q, sigma):
    """The perturbed rows' queries: the blur, or beyond sigma = 9999 (inf included) the image's mean query."""
    return mean_q(q) if is_mean(sigma) else blur(q, sigma)


# ---- the oracle's self-attention in SEG form ------------------------------------------------------------------------------
SEG = {"paths": None, "first": 0, "sigma": 100.0, "hw": None}


def grid_of(T, hw):
    """(h, w) of the level whose token count is T, halving (ceil) from the latent's (H, W)."""
    h, w = hw
    while h * w != T:
        assert h * w > T, (T, hw)
        h, w = (h + 1) // 2, (w + 1) // 2
    return h, w


def swap_attn_self(monkeypatch):
    """oracle.nets.attn_self -> a wrapper that, while SEG['paths'] is set, blurs the queries of batch rows [first, R) of the
    selected layers (fp64 blur of the fp32 queries, back to fp32) before the attention.  Undone by `monkeypatch`."""
    from oracle import nets
    orig = nets.attn_self

    def attn_self(P, path, x, heads, lora=None):
        if SEG["paths"] is None or path not in SEG["paths"]:
            return orig(P, path, x, heads, lora)
        q = nets.linear(P, path + ".to_q", x, lora)
        k = nets.linear(P, path + ".to_k", x, lora)
        v = nets.linear(P, path + ".to_v", x, lora)
        f = SEG["first"]
        R, T, C = q.shape
        h, w = grid_of(T, SEG["hw"])
        qp = seg_q(q[f:].reshape(R - f, h, w, C), SEG["sigma"]).reshape(R - f, T, C).to(q.dtype)
        return nets.linear(P, path + ".to_out.0", nets.sdpa(torch.cat([q[:f], qp]), k, v, heads), lora)
    monkeypatch.setattr(nets, "attn_self", attn_self)


def seg_unet(P, cfg, xin, t, ctx, text, tid, ip, down, mid, paths, B, sigma):
    """The main UNet on [xin rows; copies of the last B (cond) rows], the copies' selected self-attentions in SEG form
    (needs `swap_attn_self`)."""
    from oracle import nets
    R = xin.shape[0]
    c = slice(R - B, R)
    ext = lambda v: torch.cat([v, v[c]])
    SEG.update(paths=set(paths), first=R, sigma=float(sigma), hw=tuple(xin.shape[-2:]))
    try:
        return nets.unet_forward(P, cfg, ext(xin), t, ext(ctx), ext(text), ext(tid), ext(ip), [ext(d) for d in down], ext(mid))
    finally:
        SEG["paths"] = None
