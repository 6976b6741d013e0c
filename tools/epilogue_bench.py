"""The benchmark step's own launches of the 4-wave GEMM / conv kernel (csrc/gemm_conv.hip), warm, timed with device events: us per
launch and a fingerprint of the output bytes per shape.  Run once per library build and compare, or alternating through
tools/ab_lib.sh (AB_CMD="python tools/epilogue_bench.py"), as tools/g8_bench.py `ab` is:

    AB_CMD="python tools/epilogue_bench.py" bash tools/ab_lib.sh

The launches (dispatch id the chooser resolves them to): the level-2 `to_out` projection 2048 x 1280 x 1280 with residual and
LayerNorm partials (55), the level-2 FF output 2048 x 1280 x 5120 (55), the fused q|k|v projection 2048 x 3840 x 1280 with the
LayerNorm fold and the transposed V range (21), 4096 x 1280 x 1280 (54), 8192 x 640 x 640 (25), the level-0 conv 2 x 128^2
320 -> 320 with row bias + GroupNorm partials and with residual + GroupNorm partials (24), the level-2 conv 2 x 32^2
1280 -> 1280 (55), and the fused `to_q` + text / IP cross-attention launch (64 x 128 tile)."""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from instantir_amd import ops

dev = torch.device("cuda:0")
ITERS, WARM, REPEATS = 200, 20, 5


def timeit(fn):
    """Median over REPEATS windows of ITERS back-to-back launches (us per launch)."""
    for _ in range(WARM):
        fn()
    ts = []
    for _ in range(REPEATS):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(ITERS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / ITERS * 1e3)
    return sorted(ts)[len(ts) // 2], min(ts), max(ts)


def sha(*ts):
    h = hashlib.sha1()
    for t in ts:
        h.update(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()[:12]


def resolved(M, N, K, tr_from=None):
    """The dispatch id the library resolves a tile = 0 launch of this shape to (nothing is launched; a conv resolves as the GEMM of
    its M x Cout x k*k*Cin, which the 8-wave kernel never takes)."""
    import ctypes
    from instantir_amd import lib
    d = lib.GemmDesc()
    d.A, d.W, d.C = 1 << 20, 2 << 20, 3 << 20           # never dereferenced
    d.lda, d.ldc, d.M, d.N, d.K = K, N, M, N, K
    if tr_from is not None:
        d.Ct, d.ldct, d.tr_from = 4 << 20, M, tr_from
    return lib.load().iir_gemm_resolve_tile(ctypes.byref(d))


def report(name, fn, *outs, shape=None, want=None):
    if shape is not None:          # the label names a build: refuse to time another one under it
        got = resolved(*shape)
        assert got == want, f"{name}: the chooser resolves {shape} to id {got}, not {want}"
    fn()
    torch.cuda.synchronize()
    fp = sha(*outs)
    med, lo, hi = timeit(fn)
    print(f"{name:58s} {med:7.2f} us  (min {lo:7.2f} max {hi:7.2f})  sha {fp}", flush=True)


def main():
    g = torch.Generator().manual_seed(15)
    rnd = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).half().to(dev)

    def lin(M, N, K):
        return rnd(M, K), rnd(N, K, scale=K ** -0.5), rnd(N), torch.empty(M, N, dtype=torch.half, device=dev)

    M, N, K = 2048, 1280, 1280
    a, w, b, o = lin(M, N, K)
    res = rnd(M, N)
    st = torch.zeros(ops.ln_parts(M, N, K), M, 2, device=dev)
    report("gemm 2048x1280x1280 bias+res+ln_out (55)", lambda: ops.gemm(a, w, o, bias=b, res=res, ln_out=st), o, st, shape=(M, N, K), want=55)
    h = o.clone()

    a5, w5, b5, o5 = lin(2048, 1280, 5120)
    report("gemm 2048x1280x5120 bias+res (55)", lambda: ops.gemm(a5, w5, o5, bias=b5, res=res), o5, shape=(2048, 1280, 5120), want=55)

    C = 1280
    wq, bq = rnd(3 * C, C, scale=C ** -0.5), rnd(3 * C)
    fold = ops.LnFold(wq.float(), (torch.randn(C, generator=g) * 0.2 + 1).half().to(dev), (torch.randn(C, generator=g) * 0.1).half().to(dev), bias=bq.float())
    qk, vt = torch.empty(M, 2 * C, dtype=torch.half, device=dev), torch.empty(C, M, dtype=torch.half, device=dev)
    report("gemm 2048x3840x1280 q|k|v ln_in+out_t (21)", lambda: ops.gemm(h, fold.w, qk, bias=fold.bias, ln_in=(st, fold.colsum, 1e-5), out_t=(vt, 2 * C)), qk, vt, shape=(M, 3 * C, C, 2 * C), want=21)

    a4, w4, b4, o4 = lin(4096, 1280, 1280)
    r4 = rnd(4096, 1280)
    report("gemm 4096x1280x1280 bias+res (54)", lambda: ops.gemm(a4, w4, o4, bias=b4, res=r4), o4, shape=(4096, 1280, 1280), want=54)

    a6, w6, b6, o6 = lin(8192, 640, 640)
    r6 = rnd(8192, 640)
    report("gemm 8192x640x640 bias+res (25)", lambda: ops.gemm(a6, w6, o6, bias=b6, res=r6), o6, shape=(8192, 640, 640), want=25)

    R, H, Cc = 2, 128, 320
    x, wc, bc = rnd(R, H, H, Cc), rnd(Cc, 3, 3, Cc, scale=(9 * Cc) ** -0.5), rnd(Cc)
    oc = torch.empty(R * H * H, Cc, dtype=torch.half, device=dev)
    rb, rc = rnd(R, Cc), rnd(R * H * H, Cc)
    p = torch.zeros(R * H * H // 64, Cc, 2, device=dev)
    assert ops.gn_supported(R * H * H, Cc, 9 * Cc, True)
    report("conv 2x128^2 320->320 bias+rowbias+gn_out (24)", lambda: ops.conv2d(x, wc, oc, bias=bc, rowbias=rb, rows_per_rb=H * H, gn_out=p), oc, p, shape=(R * H * H, Cc, 9 * Cc), want=24)
    report("conv 2x128^2 320->320 bias+res+gn_out (24)", lambda: ops.conv2d(x, wc, oc, bias=bc, res=rc, gn_out=p), oc, p, shape=(R * H * H, Cc, 9 * Cc), want=24)

    R, H, Cc = 2, 32, 1280
    x2, wc2, bc2 = rnd(R, H, H, Cc), rnd(Cc, 3, 3, Cc, scale=(9 * Cc) ** -0.5), rnd(Cc)
    oc2 = torch.empty(R * H * H, Cc, dtype=torch.half, device=dev)
    rb2 = rnd(R, Cc)
    report("conv 2x32^2 1280->1280 bias+rowbias (55)", lambda: ops.conv2d(x2, wc2, oc2, bias=bc2, rowbias=rb2, rows_per_rb=H * H), oc2, shape=(R * H * H, Cc, 9 * Cc), want=55)

    Rx, T, heads, tk, ti = 2, 1024, 20, 77, 16
    Cx, Mx = heads * 64, Rx * T
    ax, wx, bx = rnd(Mx, Cx), rnd(Cx, Cx, scale=Cx ** -0.5 * ops.attn_q_factor()), rnd(Cx, scale=0.3 * ops.attn_q_factor())
    segs = []
    for L in (tk, ti):
        tp = (L + 7) // 8 * 8
        vtx = torch.zeros(Cx, Rx * tp, dtype=torch.half, device=dev)
        v = rnd(Rx, L, Cx)
        for r in range(Rx):
            vtx[:, r * tp:r * tp + L] = v[r].T
        segs.append((rnd(Rx * L, Cx), L, vtx, tp, L))
    ox = torch.empty(Mx, Cx, dtype=torch.half, device=dev)
    report("gemm 2048x1280x1280 to_q + cross-attention (64x128)", lambda: ops.gemm(ax, wx, ox, bias=bx, epi=ops.EPI_XATTN, xattn=(segs, T)), ox)


if __name__ == "__main__":
    main()
