"""Bits of the MFMA GEMM / implicit-GEMM convolution launches, recorded through `ops.gemm`, `ops.gemm_fp8` and `ops.conv2d`.

    python tests/golden/make_gemm_conv_bits.py <commit id of the recording checkout> [path]      # on an MI355X

`replay()` launches every build of `gemm_kernel` that `launch()` in csrc/gemm_conv.hip can instantiate and `dispatch()` can
reach (forced dispatch ids), the three `gemm8_kernel` builds, and the tile = 0 launches of every epilogue / output form, on
seeded inputs.  Every output buffer is allocated wider and longer than the view the launch writes and pre-filled with a
constant; what is stored is the SHA-256 of the WHOLE buffer, so a changed bit and a stray write both show.

The committed gemm_conv_bits.npz is never written by the code under test: it was written by the library built from the parent of
the commit that took two-slice split-K out of the kernels (every GEMM kernel got new machine code there), in a separate
checkout of that parent with this file copied in; the parent's commit id is stored under `PARENT_KEY`.
tests/test_kernels_gpu.py replays the cases on the current library and asserts equality, key for key.

Shapes: the smallest that reach every path.  G1 = 300 x 336 x 320 is ragged in M and N for every tile shape, G2 = 512 x 640 x 320
is whole tiles for every one; K is 5 K tiles, so the deepest ring (4) refills every buffer (the all-fp8 form: 640 fp8 bytes).
Conv: 3 x 3, R = 2, 12 x 12, Cin 64 -> Cout 160 (9 K tiles, 288 rows).  The one build no launch can reach is the conv form of
the 64 x 128 cross-attention tile (dispatch() refuses it).
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "gemm_conv_bits.npz")
PARENT_KEY = "recorded_by_commit"

FILL = 7.0
G1, G2 = (300, 336, 320), (512, 640, 320)
G8 = (256, 1280, 320)
CONV = dict(R=2, H=12, Cin=64, Cout=160)
F16_GEMM_IDS = [21, 31, 22, 23, 24, 34, 25, 35, 54, 55, 65, 75, 26, 36]
F16_CONV_IDS = [21, 31, 22, 23, 24, 34, 25, 35, 54, 55, 26, 36]          # loader waves: the conv exists with the 3-deep ring only
BF16_IDS = [21, 22, 23, 24, 25]
W8_IDS = [21, 22, 23, 24, 25, 35]
F8_IDS = [21, 22, 23, 24, 25, 35, 55]


def replay():
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from instantir_amd import lib, ops
    lib.load()
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(20261017)
    out = {}

    def rand(*shape, scale=1.0, dtype=torch.float16):
        return torch.from_numpy((rng.standard_normal(shape) * scale).astype(np.float32)).to(dtype).to(dev)

    def wide(t, extra=8):
        """The same values as a view of a buffer with a longer row (exercises lda / ldx)."""
        big = torch.zeros(*t.shape[:-1], t.shape[-1] + extra, dtype=t.dtype, device=dev)
        big[..., :t.shape[-1]] = t
        return big[..., :t.shape[-1]]

    def buf(rows, cols, dtype=torch.float16):
        """(whole buffer, the view a launch writes): 3 rows and 8 columns of margin, constant fill."""
        big = torch.full((rows + 3, cols + 8), FILL, dtype=dtype, device=dev)
        return big, big[:rows, :cols]

    def stats(*shape):
        """fp32 statistics buffer (must be contiguous): the view is the head of a longer flat buffer."""
        n = int(np.prod(shape))
        big = torch.full((n + 64,), FILL, dtype=torch.float32, device=dev)
        return big, big[:n].view(*shape)

    def record(key, *bufs):
        torch.cuda.synchronize()
        for i, b in enumerate(bufs):
            a = b.detach().contiguous().view(torch.uint8).cpu().numpy()
            k = key if len(bufs) == 1 else f"{key}.{i}"
            assert k not in out, k
            out[k] = np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8)

    # ---- operands (drawn once, in this order) ---------------------------------------------------------------------------------
    gemm_in = {}
    for tag, (M, N, K) in (("G1", G1), ("G2", G2), ("G8", G8)):
        for dn, dt in (("f16", torch.float16), ("bf16", torch.bfloat16)):
            if dn == "bf16" and tag == "G8":
                continue
            gemm_in[tag, dn] = dict(a=wide(rand(M, K, dtype=dt)), w=rand(N, K, scale=K ** -0.5, dtype=dt), bias=rand(N, dtype=dt),
                                    rowbias=rand((M + 3) // 4, N, dtype=dt), res=rand(M, N, dtype=dt), res_half=rand(M, N // 2, dtype=dt))
    fp8_in = {}
    for tag, (M, N, K) in (("G1", G1), ("G2", G2), ("G8", G8)):
        a8, sa = ops.quantize_fp8_tensor(rand(M, 2 * K))                       # 640 fp8 bytes of K
        w8 = ops.Fp8Weight(*ops.quantize_fp8_rows(rand(N, 2 * K, scale=(2 * K) ** -0.5)))
        w8h = ops.Fp8Weight(*ops.quantize_fp8_rows(rand(N, K, scale=K ** -0.5)))      # fp8 weights, fp16 activations
        fp8_in[tag] = dict(a8=a8, sa=sa, w8=w8, w8h=w8h)
    R, H, Cin, Cout = CONV["R"], CONV["H"], CONV["Cin"], CONV["Cout"]
    conv_in = {}
    for dn, dt in (("f16", torch.float16), ("bf16", torch.bfloat16)):
        conv_in[dn] = dict(x=wide(rand(R, H, H, Cin, dtype=dt), 64), w=rand(Cout, 3, 3, Cin, scale=(9 * Cin) ** -0.5, dtype=dt),
                           w1=rand(Cout, 1, 1, Cin, scale=Cin ** -0.5, dtype=dt), bias=rand(Cout, dtype=dt), rowbias=rand(R, Cout, dtype=dt),
                           res=rand(R * H * H, Cout, dtype=dt), res_half=rand(R * H * H, Cout // 2, dtype=dt))

    def gemm_full(key, tag, dn, tile, **kw):          # bias + row bias + residual + SiLU
        i = gemm_in[tag, dn]
        M, N = i["res"].shape
        big, o = buf(M, N, i["a"].dtype)
        ops.gemm(i["a"], kw.pop("w", i["w"]), o, bias=i["bias"], rowbias=i["rowbias"], rows_per_rb=4, res=i["res"], act=ops.ACT_SILU, tile=tile, **kw)
        record(key, big)

    def gemm_geglu(key, tag, dn, tile, **kw):
        i = gemm_in[tag, dn]
        M, N = i["res"].shape
        big, o = buf(M, N // 2, i["a"].dtype)
        ops.gemm(i["a"], kw.pop("w", i["w"]), o, bias=i["bias"], epi=ops.EPI_GEGLU, tile=tile, **kw)
        record(key, big)

    def gemm_f8(key, tag, tile, geglu):
        i, f = gemm_in[tag, "f16"], fp8_in[tag]
        M, N = i["res"].shape
        big, o = buf(M, N // 2 if geglu else N)
        if geglu:
            ops.gemm_fp8(f["a8"], f["w8"], o, a_scale=f["sa"], bias=i["bias"], epi=ops.EPI_GEGLU, tile=tile)
        else:
            ops.gemm_fp8(f["a8"], f["w8"], o, a_scale=f["sa"], bias=i["bias"], res=i["res"], act=ops.ACT_SILU, tile=tile)
        record(key, big)

    def conv(key, dn, tile, **kw):                    # 3x3, bias + per-image row bias + residual + SiLU unless told otherwise
        i = conv_in[dn]
        ks, stride, ups = kw.get("ksize", 3), kw.get("stride", 1), kw.get("upsample", False)
        Hi = 2 * H if ups else H
        Ho = (Hi + 2 * (ks // 2) - ks) // stride + 1
        Mo = R * Ho * Ho
        big, o = buf(Mo, Cout, i["x"].dtype)
        res = i["res"][:Mo] if Mo <= R * H * H else None
        ops.conv2d(i["x"], i["w1"] if ks == 1 else i["w"], o, bias=i["bias"], rowbias=i["rowbias"], rows_per_rb=Ho * Ho, res=res,
                   act=ops.ACT_SILU, tile=tile, **kw)
        record(key, big)

    # ---- every build, by forced dispatch id -------------------------------------------------------------------------------------
    for t in [0] + F16_GEMM_IDS:
        gemm_full(f"gemm.f16.G1.full.tile{t}", "G1", "f16", t)
        gemm_geglu(f"gemm.f16.G2.geglu.tile{t}", "G2", "f16", t)
    gemm_geglu("gemm.f16.G1.geglu.tile90", "G1", "f16", 90)
    gemm_geglu("gemm.f16.G2.geglu.tile90", "G2", "f16", 90)
    for t in [0] + BF16_IDS:
        gemm_full(f"gemm.bf16.G1.full.tile{t}", "G1", "bf16", t)
        gemm_geglu(f"gemm.bf16.G2.geglu.tile{t}", "G2", "bf16", t)
    for t in [0] + W8_IDS:
        for tag, fn, what in (("G1", gemm_full, "full"), ("G2", gemm_geglu, "geglu")):
            w8h = fp8_in[tag]["w8h"]
            fn(f"gemm.w8.{tag}.{what}.tile{t}", tag, "f16", t, w=w8h.q, wscale=w8h.scale)
    for t in [0] + F8_IDS:
        gemm_f8(f"gemm.f8.G1.full.tile{t}", "G1", t, False)
        gemm_f8(f"gemm.f8.G2.geglu.tile{t}", "G2", t, True)
    for t in [0] + F16_CONV_IDS:
        conv(f"conv.f16.full.tile{t}", "f16", t)
    for t in [0] + BF16_IDS:
        conv(f"conv.bf16.full.tile{t}", "bf16", t)
    i = conv_in["f16"]                                  # id 90 (256 x 320, paired epilogues only): SFT, h * (gamma + 1) + beta
    big, o = buf(R * H * H, Cout // 2)
    ops.conv2d(i["x"], i["w"], o, bias=i["bias"], res=i["res_half"], epi=ops.EPI_SFT, tile=90)
    record("conv.f16.sft.tile90", big)
    big, o = buf(R * H * H, Cout // 2)
    ops.conv2d(i["x"], i["w"], o, bias=i["bias"], res=i["res_half"], epi=ops.EPI_SFT, tile=0)
    record("conv.f16.sft.tile0", big)

    # ---- the 8-wave kernel of gemm8.hip: 256 x 320 (91), 256 x 256 (92), all-fp8 (91) ------------------------------------------
    i = gemm_in["G8", "f16"]
    M, N, _ = G8
    for t in (91, 92):
        big, o = buf(M, N)
        ops.gemm(i["a"], i["w"], o, bias=i["bias"], res=i["res"], tile=t)
        record(f"gemm8.f16.res.tile{t}", big)
        gemm_geglu(f"gemm8.f16.geglu.tile{t}", "G8", "f16", t)
    big, o = buf(M, N)
    ops.gemm_fp8(fp8_in["G8"]["a8"], fp8_in["G8"]["w8"], o, a_scale=fp8_in["G8"]["sa"], bias=i["bias"], res=i["res"], tile=91)
    record("gemm8.f8.res.tile91", big)
    gemm_f8("gemm8.f8.geglu.tile91", "G8", 91, True)

    # ---- tile = 0: every other epilogue / output form ---------------------------------------------------------------------------
    conv("conv.f16.stride2.tile0", "f16", 0, stride=2)
    conv("conv.f16.upsample.tile0", "f16", 0, upsample=True)
    conv("conv.f16.1x1.tile0", "f16", 0, ksize=1)

    M, C, N = 512, 320, 640                            # ln_out (producer of LayerNorm partials) feeding ln_in
    a0, w0, res = rand(M, C), rand(C, C, scale=C ** -0.5), rand(M, C)
    w, b, colsum = rand(N, C, scale=C ** -0.5), rand(N), rand(N, dtype=torch.float32)
    parts = ops.ln_parts(M, C, C)
    assert parts > 0, "the producer shape must leave LayerNorm partials"
    hbig, h = buf(M, C)
    sbig, st = stats(parts, M, 2)
    ops.gemm(a0, w0, h, res=res, ln_out=st)
    obig, o = buf(M, N)
    ops.gemm(h, w, o, bias=b, ln_in=(st, colsum, 1e-5))
    gbig, o2 = buf(M, N // 2)
    ops.gemm(h, w, o2, bias=b, epi=ops.EPI_GEGLU, ln_in=(st, colsum, 1e-5))
    record("gemm.f16.ln_out_ln_in.tile0", hbig, sbig, obig, gbig)

    M, N, K = 256, 640, 320                            # gn_out (GroupNorm partials) from a GEMM and from a conv
    assert ops.gn_supported(M, N, K) and ops.gn_supported(2 * 16 * 16, 320, 9 * 64, True), "shapes must leave GroupNorm partials"
    big, o = buf(M, N)
    pbig, p = stats(M // 64, N, 2)
    ops.gemm(rand(M, K), rand(N, K, scale=K ** -0.5), o, bias=rand(N), res=rand(M, N), gn_out=p)
    record("gemm.f16.gn_out.tile0", big, pbig)
    big, o = buf(512, 320)
    pbig, p = stats(512 // 64, 320, 2)
    ops.conv2d(rand(2, 16, 16, 64), rand(320, 3, 3, 64, scale=1 / 24), o, bias=rand(320), rowbias=rand(2, 320), rows_per_rb=256,
               res=rand(512, 320), gn_out=p)
    record("conv.f16.gn_out.tile0", big, pbig)

    M, C, K = 256, 160, 320                            # out_t: q | k row-major, the V third transposed (one tile straddles tr_from)
    qbig, qk = buf(M, 2 * C)
    vbig, vt = buf(C, M)
    ops.gemm(rand(M, K), rand(3 * C, K, scale=K ** -0.5), qk, bias=rand(3 * C), out_t=(vt, 2 * C))
    record("gemm.f16.out_t.tile0", qbig, vbig)

    i = gemm_in["G1", "f16"]                           # fp32 output
    big, o = buf(G1[0], G1[1], torch.float32)
    ops.gemm(i["a"], i["w"], o, out_scale=0.5)
    record("gemm.f16.c_f32.tile0", big)

    assert ops.fp8_out_supported(G2[0], G2[1], 2 * G2[2]) and ops.fp8_out_supported(G2[0], G2[1], 2 * G2[2], True)
    f, i = fp8_in["G2"], gemm_in["G2", "f16"]          # fp8 output of the all-fp8 form, plain and GEGLU
    big, o = buf(G2[0], G2[1], torch.uint8)
    ops.gemm_fp8(f["a8"], f["w8"], o, a_scale=f["sa"], bias=i["bias"], res=i["res"])
    gbig, o2 = buf(G2[0], G2[1] // 2, torch.uint8)
    ops.gemm_fp8(f["a8"], f["w8"], o2, a_scale=f["sa"], bias=i["bias"], epi=ops.EPI_GEGLU)
    record("gemm.f8.c_fp8.tile0", big, gbig)

    Rx, T, heads, K, tk, ti = 3, 64, 4, 192, 13, 4      # to_q + text / IP cross-attention in one launch (smallest shape of its test)
    C, M = heads * 64, Rx * T
    a, w, b = rand(M, K), rand(C, K, scale=K ** -0.5 * ops.attn_q_factor()), rand(C, scale=0.3 * ops.attn_q_factor())
    segs = []
    for L in (tk, ti):
        tp = (L + 7) // 8 * 8
        vt = torch.zeros(C, Rx * tp, dtype=torch.half, device=dev)
        v = rand(Rx, L, C)
        for r in range(Rx):
            vt[:, r * tp:r * tp + L] = v[r].T
        segs.append((rand(Rx * L, C), L, vt, tp, L))
    big, o = buf(M, C)
    ops.gemm(a, w, o, bias=b, epi=ops.EPI_XATTN, xattn=(segs, T))
    record("gemm.f16.xattn", big)
    return out


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    path = sys.argv[2] if len(sys.argv) > 2 else PATH
    bits = replay()
    bits[PARENT_KEY] = np.frombuffer(sys.argv[1].encode(), dtype=np.uint8)
    np.savez_compressed(path, **bits)
    print(f"wrote {path}: {len(bits) - 1} buffers recorded by {sys.argv[1]}, {os.path.getsize(path)} bytes")
