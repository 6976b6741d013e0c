"""Thin launch wrappers: torch CUDA tensors in, one C-ABI call out.  torch is used for device
memory and the current stream only; no arithmetic happens here.

All activations are fp16, channel/feature dimension contiguous.  Matrices are 2-D views whose
row stride may exceed the width (column slices of wider buffers are passed as views).
"""
from __future__ import annotations

import ctypes as C

import torch

from . import lib as L
from .images import check_crop
from .lib import ACT_GELU, ACT_NONE, ACT_QUICKGELU, ACT_SILU, EPI_GEGLU, EPI_PLAIN, EPI_SFT, EPI_XATTN  # noqa: F401


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


_DT = {torch.float16: L.MACROS["IIR_DT_F16"], torch.bfloat16: L.MACROS["IIR_DT_BF16"]}


def _chk2d(t, name, dtype=torch.float16):
    """2-D CUDA tensor of `dtype` (fp16 unless the call runs the bf16 build: the VAE) with unit column stride."""
    if t.dtype != dtype or t.dim() != 2 or t.stride(1) != 1 or not t.is_cuda:
        raise ValueError(f"{name}: expected a 2-D {dtype} CUDA tensor with unit column stride, got {t.dtype} {tuple(t.shape)} {t.stride()}")


class LaunchProfiler:
    """Optional per-launch timing of the MFMA kernels (bench.py's roofline leg): each launch is issued with a HIP
    start/stop event pair that the runtime stamps with the kernel's own begin / end timestamps on its stream
    (`iir_timing_arm`, hipExtLaunchKernelGGL).  Records (kernel class, algorithmic FLOPs, start, stop)."""

    def __init__(self):
        self.records = []
        self._pool = []

    def events(self):
        h = L.load()
        e0, e1 = h.iir_timing_event_create(), h.iir_timing_event_create()
        if not e0 or not e1:
            raise L.HipLibraryError("hipEventCreate failed")
        self._pool += [e0, e1]
        return e0, e1

    def summary(self):
        torch.cuda.synchronize()
        h = L.load()
        out = {}
        us = C.c_float()
        for cls, flops, e0, e1, nbytes in self.records:
            L.check(h.iir_timing_elapsed_us(e0, e1, C.byref(us)), "iir_timing_elapsed_us")
            d = out.setdefault(cls, {"launches": 0, "ms": 0.0, "flops": 0.0, "bytes": 0.0})
            d["launches"] += 1
            d["ms"] += us.value * 1e-3
            d["flops"] += flops
            d["bytes"] += nbytes
        for e in self._pool:
            h.iir_timing_event_destroy(e)
        self._pool = []
        return out


PROFILER = None     # set to a LaunchProfiler to time gemm / conv / attention launches

_TILE_NAMES = {1: "128x128", 2: "128x64", 3: "64x64", 4: "128x160", 5: "64x160", 6: "256x128", 0: "256x320"}   # 0: tile id 90


def auto_tile(M, N, paired=False, K=0):
    """The tile `tile=0` resolves to (single source of truth: pick_tile() in csrc/gemm_conv.hip)."""
    return L.load().iir_gemm_pick_tile(M, N, K, int(paired))


class _Timed:
    def __init__(self, cls, flops, nbytes=0.0):
        self.cls, self.flops, self.nbytes = cls, flops, nbytes      # algorithmic FLOPs and bytes (each operand once)

    def __enter__(self):
        if PROFILER is not None:
            e0, e1 = PROFILER.events()
            L.check(L.load().iir_timing_arm(e0, e1), "iir_timing_arm")
            PROFILER.records.append((self.cls, self.flops, e0, e1, self.nbytes))

    def __exit__(self, *a):
        pass


_zero_pages = {}


def zero_page(device):
    z = _zero_pages.get(device)
    if z is None:
        z = torch.zeros(256, dtype=torch.float16, device=device)
        _zero_pages[device] = z
    return z


FP8_MAX = 448.0          # largest finite E4M3 (OCP) value


class Fp8Weight:
    """A linear layer's weight as fp8-E4M3 bytes + per-output-channel fp32 scale; `gemm` accepts it in place of `w`."""

    def __init__(self, q, scale):
        self.q, self.scale = q, scale
        self.shape = q.shape

    def numel(self):
        return self.q.numel() // 2          # in fp16-element units: what the weight-arena bookkeeping counts

    def data_ptr(self):
        return self.q.data_ptr()


def quantize_fp8_rows(w):
    """Per-output-channel E4M3 quantisation of a weight matrix (N, K): returns (bytes (N, K) as torch.float8_e4m3fn,
    fp32 scale (N,)) with w ~= bytes * scale[:, None].  Pack-time plumbing for `gemm(..., wscale=)`."""
    w32 = w.float()
    scale = (w32.abs().amax(dim=1).clamp_min(1e-12) / FP8_MAX).contiguous()
    q = (w32 / scale[:, None]).clamp(-FP8_MAX, FP8_MAX).to(torch.float8_e4m3fn).contiguous()
    return q, scale


_FP8_DTYPES = (torch.float8_e4m3fn, torch.uint8)


def gemm_fp8(a8, w8, out, a_scale=1.0, bias=None, res=None, epi=EPI_PLAIN, act=ACT_NONE, tile=0, prefetch=None, out_t=None):
    """out = epi((a8 @ w8.q.T) * w8.scale[None, :] * a_scale ...): BOTH operands fp8-E4M3 (`iir_gemm_desc.a_fp8`).
    a8 (M, K) torch.float8_e4m3fn (or its bytes) view with a 16-byte-aligned row stride, K % 128 == 0; w8 an `Fp8Weight`;
    out / bias / res fp16.  One K tile is 128 K values = the same 128-byte rows the fp16 path stages for 64."""
    if not isinstance(w8, Fp8Weight):
        raise ValueError("gemm_fp8: w8 must be an Fp8Weight")
    if a8.dtype not in _FP8_DTYPES or a8.dim() != 2 or a8.stride(1) != 1 or not a8.is_cuda:
        raise ValueError("gemm_fp8: a8 must be a 2-D CUDA view of torch.float8_e4m3fn (or its bytes) with contiguous rows")
    M, K = a8.shape
    N = w8.q.shape[0]
    if w8.q.shape[1] != K or K % 128 or a8.stride(0) % 16:
        raise ValueError("gemm_fp8: K must match, K % 128 == 0, row stride % 16 == 0")
    dt = torch.float16
    c_fp8 = out.dtype in _FP8_DTYPES            # the output is the NEXT all-fp8 GEMM's A operand: stored as E4M3 bytes (fp16 rounding first)
    if c_fp8:
        if out.dim() != 2 or out.stride(1) != 1 or out.stride(0) % 8 or not out.is_cuda:
            raise ValueError("gemm_fp8: an fp8 `out` needs contiguous rows with a stride % 8 == 0")
    else:
        _chk2d(out, "out", dt)
    n_out = (N if epi == EPI_PLAIN else N // 2) if out_t is None else out_t[1]
    if out.shape != (M, n_out):
        raise ValueError(f"out shape {tuple(out.shape)} != {(M, n_out)}")
    for t_, n_ in ((bias, "bias"), (res, "res")):
        if t_ is not None and t_.dtype != dt:
            raise ValueError(f"{n_}: fp16 expected")
    d = L.GemmDesc()
    d.c_fp8 = int(c_fp8)
    if out_t is not None:
        _fill_out_t(d, out_t, dt, M, N, c_fp8, "out_t: fp16 (N - tr_from, M), with an fp16 `out`")
    d.A, d.lda = a8.data_ptr(), a8.stride(0)
    d.W, d.wscale = w8.q.data_ptr(), w8.scale.data_ptr()
    d.C, d.ldc = out.data_ptr(), out.stride(0)
    d.M, d.N, d.K = M, N, K
    d.bias = _p(bias)
    if res is not None:
        _chk2d(res, "res", dt)
        d.res, d.ldr = res.data_ptr(), res.stride(0)
    d.epi, d.act, d.out_scale, d.tile = epi, act, 1.0, tile
    d.dtype, d.a_fp8, d.a_scale = _DT[dt], 1, float(a_scale)
    if prefetch is not None:
        d.prefetch, d.prefetch_bytes = prefetch
    t_name = tile if tile else auto_tile(M, N, epi != EPI_PLAIN, K)
    cls = "gemm_kernel<%s,gemm-f8>" % _TILE_NAMES[t_name % 10]
    if tile == 91 or (PROFILER is not None and tile == 0 and L.load().iir_gemm_resolve_tile(C.byref(d)) == 91):
        cls = "gemm8_kernel<256x320,gemm-f8>"
    with _Timed(cls, 2.0 * M * N * K, 1.0 * (M * K + N * K) + 2.0 * M * n_out * (2 if res is not None else 1)):
        L.check(L.load().iir_gemm_f16(C.byref(d), _stream()), "iir_gemm_f16")
    return out


def fp8_out_supported(M, N, K, paired=False):
    """Can the all-fp8 launch of (M, N, K) store its result as fp8 bytes (an fp8 `out` of `gemm_fp8`)?"""
    return bool(L.load().iir_gemm_fp8_out_supported(M, N, K, int(paired)))


def quantize_fp8_tensor(x):
    """Per-tensor E4M3 quantisation of an activation matrix: (bytes as torch.float8_e4m3fn, scale) with x ~= bytes * scale."""
    x32 = x.float()
    scale = float(x32.abs().amax().clamp_min(1e-12) / FP8_MAX)
    return (x32 / scale).clamp(-FP8_MAX, FP8_MAX).to(torch.float8_e4m3fn).contiguous(), scale


class LnFold:
    """A LayerNorm folded into the nn.Linear that follows it (weight-pack time): `w` = W . diag(gamma) (fp16, or an Fp8Weight of
    it), `colsum[n]` = sum_k w[n][k] in fp32 (of the STORED values, so the mean term cancels exactly), `bias` = b + W . beta."""

    def __init__(self, weight, gamma, beta, bias=None, eps=1e-5, fp8=False, pair=None):
        w32 = weight.float() * gamma.float()[None, :]
        b32 = weight.float() @ beta.float() + (bias.float() if bias is not None else 0.0)
        if pair is not None:                       # GEGLU: value rows | gate rows interleaved like the weight (packing.pair_rows)
            n = w32.shape[0] // 2
            w32, b32 = pair(w32[:n], w32[n:]), pair(b32[:n], b32[n:])
        w16 = w32.to(torch.float16).contiguous()
        if fp8:
            q, sc = quantize_fp8_rows(w16)
            self.w = Fp8Weight(q, sc)
            self.colsum = (q.float().sum(dim=1) * sc).contiguous()
        else:
            self.w = w16
            self.colsum = w16.float().sum(dim=1).contiguous()
        self.bias = b32.to(torch.float16).contiguous()
        self.eps = float(eps)


def ln_parts(M, N, K):
    """Partials per row the plain-epilogue, tile = 0 launch of (M, N, K) leaves in `ln_out` (0: it cannot)."""
    return L.load().iir_gemm_ln_parts(M, N, K)


GN_PARTIALS_MAX = 20 * 256          # slabs x channels-per-group one (image, group) of iir_groupnorm_from_partials may hold (csrc/norm.hip)


def gn_supported(M, N, K, conv=False):
    """Can the tile = 0 launch of (M, N, K) leave GroupNorm partials (`gn_out=`)?"""
    return bool(L.load().iir_gemm_gn_supported(M, N, K, int(conv)))


def _chk_gn_out(gn_out, M, N):
    """GroupNorm partials of a producing launch: fp32 (M / 64, N, 2), contiguous (`iir_gemm_desc.gn_stats_out`)."""
    if gn_out.dtype != torch.float32 or not gn_out.is_contiguous() or M % 64 or tuple(gn_out.shape) != (M // 64, N, 2):
        raise ValueError(f"gn_out: contiguous fp32 ({M} // 64, {N}, 2) with M % 64 == 0, got {tuple(gn_out.shape)} {gn_out.dtype}")


def _fill_operands(d, dt, M, N, rowbias, rows_per_rb, res, prefetch, gn_out):
    """The optional operands `GemmDesc` and `ConvDesc` name alike: per-image row bias, residual, GroupNorm partials of the
    (M, N) output, weight prefetch range."""
    if rowbias is not None:
        _chk2d(rowbias, "rowbias", dt)
        d.rowbias, d.ldrb, d.rows_per_rb = rowbias.data_ptr(), rowbias.stride(0), rows_per_rb
    if res is not None:
        _chk2d(res, "res", dt)
        d.res, d.ldr = res.data_ptr(), res.stride(0)
    if gn_out is not None:
        _chk_gn_out(gn_out, M, N)
        d.gn_stats_out = gn_out.data_ptr()
    if prefetch is not None:
        d.prefetch, d.prefetch_bytes = prefetch


def _fill_out_t(d, out_t, dt, M, N, refuse, msg):
    """out_t = (Ct, tr_from): output columns >= tr_from leave transposed, to Ct[n - tr_from, m] (the V third of q|k|v)."""
    ct, tr_from = out_t
    _chk2d(ct, "out_t", dt)
    if refuse or ct.shape[0] < N - tr_from or ct.shape[1] < M:
        raise ValueError(msg)
    d.Ct, d.ldct, d.tr_from = ct.data_ptr(), ct.stride(0), tr_from


def _fill_kv(table, kv):
    """The K / V^T segment table (`iir_attn_kv` entries) of `attention` and of `gemm(xattn=)`."""
    for i, (k, k_rows, vt, vbs, tkv) in enumerate(kv):
        _chk2d(k, "k"); _chk2d(vt, "vt")
        e = table[i]
        e.K, e.ldk, e.k_batch_stride = k.data_ptr(), k.stride(0), k_rows * k.stride(0)
        e.Vt, e.ldvt, e.vt_batch_stride = vt.data_ptr(), vt.stride(0), vbs
        e.Tkv = tkv


def gemm(a, w, out, bias=None, rowbias=None, rows_per_rb=1, res=None, epi=EPI_PLAIN, act=ACT_NONE, out_scale=1.0,
         tile=0, prefetch=None, out_t=None, wscale=None, ln_out=None, ln_in=None, gn_out=None, xattn=None):
    """out = epi(a @ w.T).  a (M,K) view, w (N,K) contiguous, out (M,N) view ((M,N/2) for paired epilogues).
    out_t = (Ct, tr_from): output columns >= tr_from go, transposed, to Ct[n - tr_from, m]; `out` then is (M, tr_from).
    wscale (fp32 (N,)): `w` holds fp8-E4M3 bytes (torch.float8_e4m3fn / uint8) with that per-row scale (fp8 MFMA).
    ln_out (fp32 (parts, M, 2), parts = ln_parts(M, N, K)): also leave LayerNorm partials of the rows written.
    ln_in = (partials (parts, M, 2) fp32, colsum (N,) fp32, eps): `a` holds raw rows, `w` / `bias` are an `LnFold`'s.
    xattn = (kv, Tq) with epi = EPI_XATTN: `w` is a cross-attention q projection with `attn_q_factor()` folded in; `out` receives the
    text + IP cross-attention output of those queries (kv: two tuples as for `attention`, Tq: query rows per image).  `out_scale`
    then scales the FINISHED output, not q: out = fp16(fp16(O_text + O_ip) * out_scale), the write-out's product on the stored fp16
    tile as for every other epilogue (tests/xattn_ref.py states it; tests/test_xattn_every_case_gpu.py runs it at 0.5)."""
    dt = a.dtype
    if isinstance(w, Fp8Weight):
        w, wscale = w.q, w.scale
    if wscale is not None:
        if w.dtype not in (torch.float8_e4m3fn, torch.uint8) or w.dim() != 2 or not w.is_contiguous() or not w.is_cuda:
            raise ValueError("fp8 weights: contiguous 2-D CUDA tensor of torch.float8_e4m3fn (or its bytes)")
        if wscale.dtype != torch.float32 or wscale.numel() != w.shape[0] or not wscale.is_contiguous():
            raise ValueError("wscale: contiguous fp32 (N,)")
        if dt != torch.float16:
            raise ValueError("fp8 weights take fp16 activations")
    if dt not in _DT:
        raise ValueError(f"a: fp16 or bf16 expected, got {dt}")
    c_f32 = out.dtype == torch.float32                 # fp32 output (plain epilogue only): the VAE's attention scores
    _chk2d(a, "a", dt); _chk2d(out, "out", torch.float32 if c_f32 else dt)
    if wscale is None:
        _chk2d(w, "w", dt)
    for t_, n_ in ((bias, "bias"), (rowbias, "rowbias"), (res, "res")):
        if t_ is not None and t_.dtype != dt:
            raise ValueError(f"{n_}: dtype {t_.dtype} does not match the operands ({dt})")
    M, K = a.shape
    N = w.shape[0]
    if w.shape[1] != K or not w.is_contiguous():
        raise ValueError("w must be contiguous (N,K) with K matching a")
    n_out = (N if epi in (EPI_PLAIN, EPI_XATTN) else N // 2) if out_t is None else out_t[1]
    if out.shape != (M, n_out):
        raise ValueError(f"out shape {tuple(out.shape)} != {(M, n_out)}")
    d = L.GemmDesc()
    d.A, d.lda = a.data_ptr(), a.stride(0)
    d.W = w.data_ptr()
    d.C, d.ldc = out.data_ptr(), out.stride(0)
    d.M, d.N, d.K = M, N, K
    d.bias = _p(bias)
    _fill_operands(d, dt, M, N, rowbias, rows_per_rb, res, prefetch, gn_out)
    d.epi, d.act, d.out_scale, d.tile = epi, act, out_scale, tile
    d.dtype, d.c_f32 = _DT[dt], int(c_f32)
    if wscale is not None:
        d.wscale = wscale.data_ptr()
    if ln_out is not None:
        if ln_out.dtype != torch.float32 or not ln_out.is_contiguous() or ln_out.dim() != 3 or ln_out.shape[1:] != (M, 2) \
                or ln_out.shape[0] != ln_parts(M, N, K) or tile != 0:
            raise ValueError("ln_out: contiguous fp32 (ln_parts(M, N, K), M, 2), tile = 0")
        d.ln_stats_out = ln_out.data_ptr()
    if ln_in is not None:
        part, colsum, eps = ln_in
        if part.dtype != torch.float32 or not part.is_contiguous() or part.dim() != 3 or part.shape[1:] != (M, 2) or K % part.shape[0]:
            raise ValueError("ln_in partials: contiguous fp32 (parts, M, 2) with parts dividing K")
        if colsum.dtype != torch.float32 or colsum.numel() != N or not colsum.is_contiguous():
            raise ValueError("ln_in colsum: contiguous fp32 (N,)")
        d.ln_stats_in, d.ln_colsum, d.ln_parts, d.ln_part_cols, d.ln_eps = part.data_ptr(), colsum.data_ptr(), part.shape[0], K // part.shape[0], eps
    kv_keep = None
    if (epi == EPI_XATTN) != (xattn is not None):
        raise ValueError("epi = EPI_XATTN goes with xattn = (kv, Tq)")
    if xattn is not None:
        kvs, tq = xattn
        if len(kvs) != 2:
            raise ValueError("xattn: two K / V^T segments (text, IP tokens)")
        kv_keep = (L.AttnKV * 2)()
        _fill_kv(kv_keep, kvs)
        d.xattn_kv, d.xattn_tq = kv_keep, tq
    if xattn is not None:
        tile = 93
    elif tile == 0:       # the library decides; resolve the same choice here only to NAME the launch for the profiler
        tile = auto_tile(M, N, epi != EPI_PLAIN, K)
    if out_t is not None:
        _fill_out_t(d, out_t, dt, M, N, False, "out_t must hold (N - tr_from, M)")
    No = N // 2 if epi not in (EPI_PLAIN, EPI_XATTN) else N
    if xattn is not None:
        cls = "gemm_kernel<64x128,gemm+xattn>"
    elif PROFILER is not None and d.tile == 0 and L.load().iir_gemm_resolve_tile(C.byref(d)) in (91, 92):
        cls = "gemm8_kernel<256x%d,gemm>" % (320 if L.load().iir_gemm_resolve_tile(C.byref(d)) == 91 else 256)      # the 8-wave kernel of csrc/gemm8.hip
    else:
        cls = "gemm_kernel<%s,%s>" % (_TILE_NAMES[tile % 10], "gemm" if wscale is None else "gemm-w8")
    xa_flops = 4.0 * M * N * sum(k[4] for k in xattn[0]) if xattn is not None else 0.0
    with _Timed(cls, 2.0 * M * N * K + xa_flops,
                2.0 * (M * K + N * K * (1.0 if wscale is None else 0.5) + M * No + (M * No if res is not None else 0))):
        L.check(L.load().iir_gemm_f16(C.byref(d), _stream()), "iir_gemm_f16")
    return out


def conv2d(x, w, out, ksize=3, stride=1, upsample=False, bias=None, rowbias=None, rows_per_rb=1, res=None,
           epi=EPI_PLAIN, act=ACT_NONE, out_scale=1.0, tile=0, y_img_rows=0, res_img_rows=0, pad_mode=0, prefetch=None, gn_out=None):
    """x (R,H,W,Cin) NHWC view (pixel stride x.stride(2), image stride x.stride(0) free), w (Cout,k,k,Cin) contiguous,
    out (rows, Cout[/2]) 2-D view; image i's pixels start at row i*y_img_rows (0 = dense)."""
    R, H, Wd, Cin = x.shape
    dt = x.dtype
    if dt not in _DT or x.stride(3) != 1 or x.stride(1) != Wd * x.stride(2):
        raise ValueError("x must be an NHWC fp16 / bf16 view with dense rows (pixel and image strides are free)")
    _chk2d(out, "out", dt)
    for t_, n_ in ((w, "w"), (bias, "bias"), (rowbias, "rowbias"), (res, "res")):
        if t_ is not None and t_.dtype != dt:
            raise ValueError(f"{n_}: dtype {t_.dtype} does not match x ({dt})")
    Cout = w.shape[0]
    if tuple(w.shape[1:]) != (ksize, ksize, Cin) or not w.is_contiguous():
        raise ValueError("w must be contiguous (Cout,k,k,Cin)")
    d = L.ConvDesc()
    d.X, d.ldx = x.data_ptr(), x.stride(2)
    d.R, d.H, d.Wd, d.Cin = R, H, Wd, Cin
    d.Wt = w.data_ptr()
    d.Y, d.ldy = out.data_ptr(), out.stride(0)
    d.Cout, d.ksize, d.stride, d.upsample = Cout, ksize, stride, int(bool(upsample))
    d.bias = _p(bias)
    d.dtype = _DT[dt]
    Hi, Wi = (2 * H, 2 * Wd) if upsample else (H, Wd)
    pad2 = 1 if pad_mode == 1 else 2 * (ksize // 2)
    Mo = R * ((Hi + pad2 - ksize) // stride + 1) * ((Wi + pad2 - ksize) // stride + 1)
    _fill_operands(d, dt, Mo, Cout, rowbias, rows_per_rb, res, prefetch, gn_out)
    d.epi, d.act, d.out_scale, d.tile = epi, act, out_scale, tile
    if tile == 0:       # as in gemm(): the library decides, this only names the launch
        Kc = ksize * ksize * Cin
        tile = auto_tile(Mo, Cout, epi != EPI_PLAIN, Kc)
    d.zero_page = zero_page(x.device).data_ptr()          # (all-zero bits are zero in fp16 and bf16 alike)
    d.x_img_stride, d.y_img_rows, d.res_img_rows, d.pad_mode = x.stride(0), y_img_rows, res_img_rows, pad_mode
    Co = Cout // 2 if epi != EPI_PLAIN else Cout
    with _Timed("gemm_kernel<%s,conv>" % _TILE_NAMES[tile % 10], 2.0 * Mo * Cout * ksize * ksize * Cin,
                2.0 * (R * H * Wd * Cin + Cout * ksize * ksize * Cin + Mo * Co + (Mo * Co if res is not None else 0))):
        L.check(L.load().iir_conv2d_nhwc_f16(C.byref(d), _stream()), "iir_conv2d_nhwc_f16")
    return out


ATTN_LOG2E = 1.4426950408889634


def attn_q_factor(scale=0.125):
    """The factor a caller folds into its q-projection weights to pass `q_prescaled=True` (float32, as the kernel forms it)."""
    import numpy as np
    return float(np.float32(scale) * np.float32(ATTN_LOG2E))


def attention(q, o, kv, batch, heads, Tq, scale=0.125, causal=False, q_prescaled=False, head_dim=64, ident_from=0):
    """q, o: 2-D views (batch*Tq, heads*head_dim).  kv: list of 1-2 tuples (k2d, k_batch_rows, vt2d, vt_batch_stride, Tkv):
    k2d (batch*k_batch_rows, heads*head_dim) view, vt2d (heads*head_dim, cols) view with batch b starting at column
    b*vt_batch_stride.  head_dim 64 (the UNet, DINOv2, CLIP-B/L) runs `iir_attention_d64_f16`; 80 and 104 (CLIP ViT-H/14,
    bigG/14 vision towers) `iir_attention_f16` (no fp8 `o`).  `ident_from` > 0: batch rows [ident_from, batch) get the
    identity attention map, o = v (perturbed-attention guidance, `iir_attention_d64_ident_f16`)."""
    _chk2d(q, "q")
    d = L.AttnDesc()
    if o.dtype in _FP8_DTYPES:          # the output feeds an all-fp8 `to_out` GEMM: E4M3 bytes (rounded to fp16 first)
        if o.dim() != 2 or o.stride(1) != 1 or o.stride(0) % 4 or not o.is_cuda:
            raise ValueError("attention: an fp8 `o` needs contiguous rows with a stride % 4 == 0")
        d.o_fp8 = 1
    else:
        _chk2d(o, "o")
    d.Q, d.ldq, d.q_batch_stride = q.data_ptr(), q.stride(0), Tq * q.stride(0)
    d.O, d.ldo, d.o_batch_stride = o.data_ptr(), o.stride(0), Tq * o.stride(0)
    d.batch, d.heads, d.Tq, d.nseg, d.scale = batch, heads, Tq, len(kv), scale
    d.causal = int(bool(causal))
    d.q_prescaled = int(bool(q_prescaled))
    _fill_kv(d.kv, kv)
    if ident_from:
        if head_dim != 64:
            raise ValueError("attention: identity rows need head_dim 64")
        with _Timed("attn_kernel", 4.0 * ident_from * heads * Tq * head_dim * kv[0][4],
                    2.0 * ident_from * heads * head_dim * (2 * Tq + 2 * kv[0][4]) + 4.0 * (batch - ident_from) * heads * Tq * head_dim):
            L.check(L.load().iir_attention_d64_ident_f16(C.byref(d), int(ident_from), _stream()), "iir_attention_d64_ident_f16")
        return o
    with _Timed("attn_kernel", 4.0 * batch * heads * Tq * head_dim * sum(k[4] for k in kv),
                2.0 * batch * heads * head_dim * (2 * Tq + 2 * sum(k[4] for k in kv))):
        if head_dim == 64:
            L.check(L.load().iir_attention_d64_f16(C.byref(d), _stream()), "iir_attention_d64_f16")
        else:
            L.check(L.load().iir_attention_f16(C.byref(d), head_dim, _stream()), "iir_attention_f16")
    return o


def attention_1h(q, o, k, vt, vt_batch_stride, batch, Tq, Tkv, scale, bias=None):
    """Single-head attention at head_dim = q.shape[1] (128 / 256 / 512: the VAE mid block), `iir_attention_1h`: one flash-style
    launch for the whole batch.  q, o: 2-D views (batch*Tq, D); k: (batch*Tkv, D) view; vt: (D, cols) view with image b's keys
    at columns b*vt_batch_stride + [0, Tkv), readable up to roundup8(Tkv) (values at and past Tkv are ignored); bias: (D,)
    added to every output row.  fp16 or bf16, taken from the tensors."""
    dt = q.dtype
    if dt not in _DT:
        raise ValueError(f"attention_1h: fp16 or bf16 expected, got {dt}")
    for t_, n_ in ((q, "q"), (o, "o"), (k, "k"), (vt, "vt")):
        _chk2d(t_, n_, dt)
    D = q.shape[1]
    if o.shape[1] != D or k.shape[1] != D or vt.shape[0] != D:
        raise ValueError("attention_1h: q, o, k need the same width D and vt D rows")
    if q.shape[0] < batch * Tq or o.shape[0] < batch * Tq or k.shape[0] < batch * Tkv:
        raise ValueError("attention_1h: q / o need batch*Tq rows and k batch*Tkv rows")
    last = (batch - 1) * vt_batch_stride
    if last + Tkv > vt.shape[1] or last + (Tkv + 7) // 8 * 8 > vt.stride(0) or (batch > 1 and vt_batch_stride < Tkv):
        raise ValueError("attention_1h: every image's Tkv columns must lie inside vt and their roundup8(Tkv) inside a row of its buffer")
    if bias is not None and (bias.dtype != dt or bias.dim() != 1 or bias.numel() != D or not bias.is_contiguous() or not bias.is_cuda):
        raise ValueError(f"attention_1h: bias must be a contiguous {dt} CUDA vector of {D}")
    d = L.AttnDesc()
    d.Q, d.ldq, d.q_batch_stride = q.data_ptr(), q.stride(0), Tq * q.stride(0)
    d.O, d.ldo, d.o_batch_stride = o.data_ptr(), o.stride(0), Tq * o.stride(0)
    d.batch, d.heads, d.Tq, d.nseg, d.scale = batch, 1, Tq, 1, scale
    e = d.kv[0]
    e.K, e.ldk, e.k_batch_stride = k.data_ptr(), k.stride(0), Tkv * k.stride(0)
    e.Vt, e.ldvt, e.vt_batch_stride, e.Tkv = vt.data_ptr(), vt.stride(0), vt_batch_stride, Tkv
    with _Timed("attn_1h_kernel", 4.0 * batch * Tq * D * Tkv, 2.0 * batch * D * (2 * Tq + 2 * Tkv)):
        L.check(L.load().iir_attention_1h(C.byref(d), D, _DT[dt], _p(bias), _stream()), "iir_attention_1h")
    return o


_gn_ws = {}


def _gn_workspace(device, R, groups):
    """fp32 partial-sum scratch, one per (device, stream): launches on different streams may overlap."""
    need = L.load().iir_groupnorm_workspace_bytes(R, groups)
    key = (device, _stream())
    ws = _gn_ws.get(key)
    if ws is None or ws.numel() * 4 < need:
        ws = torch.empty(need // 4, dtype=torch.float32, device=device)
        _gn_ws[key] = ws
    return ws


def gn_workspace(device, R, groups=32):
    """Caller-owned fp32 scratch for `groupnorm` (one per concurrently running network)."""
    return torch.empty(L.load().iir_groupnorm_workspace_bytes(R, groups) // 4, dtype=torch.float32, device=device)


def _chk_cols(who, Cc, **vecs):
    """Every given per-channel operand (a vector, or rows of modulation) has `Cc` unit-stride columns."""
    for name, t in vecs.items():
        if t is not None and (t.dim() < 1 or t.shape[-1] != Cc or t.stride(-1) != 1):
            raise ValueError(f"{who}: {name} needs {Cc} contiguous columns, got {tuple(t.shape)} {t.stride()}")


def groupnorm(x, out, R, HW, gamma, beta, eps, silu, groups=32, ws=None, partials=None):
    """x, out: 2-D views (R*HW, C).  `ws`: scratch from gn_workspace() (a shared per-stream one if omitted).
    `partials` (fp32 (R*HW / 64, C, 2)): the statistics the launch that PRODUCED x left (`gn_out=` of gemm / conv2d): no
    statistics pass over x."""
    dt = x.dtype
    if x.dim() != 2 or tuple(out.shape) != tuple(x.shape) or x.shape[0] != R * HW:
        raise ValueError(f"groupnorm: x and out are ({R} * {HW}, C), got {tuple(x.shape)} and {tuple(out.shape)}")
    Cc = x.shape[1]
    _chk_cols("groupnorm", Cc, gamma=gamma, beta=beta)
    _chk2d(x, "x", dt if dt in _DT else torch.float16); _chk2d(out, "out", dt)
    if gamma.dtype != dt or beta.dtype != dt:
        raise ValueError(f"gamma / beta must have the activations' dtype ({dt})")
    if ws is None:
        ws = _gn_workspace(x.device, R, groups)
    if partials is not None:
        _chk_gn_out(partials, R * HW, Cc)
        if HW % 64 or (HW // 64) * (Cc // groups) > GN_PARTIALS_MAX:
            raise ValueError(f"groupnorm(partials=): images of whole 64-row slabs and at most {GN_PARTIALS_MAX} partials per (image, group); "
                             f"got HW={HW}, {Cc // groups} channels per group")
        L.check(L.load().iir_groupnorm_from_partials(partials.data_ptr(), Cc, x.data_ptr(), x.stride(0), out.data_ptr(), out.stride(0),
                                                     R, HW, Cc, groups, gamma.data_ptr(), beta.data_ptr(), eps, int(silu), ws.data_ptr(),
                                                     ws.numel() * 4, _DT[dt], _stream()), "iir_groupnorm_from_partials")
        return out
    L.check(L.load().iir_groupnorm_nhwc(x.data_ptr(), x.stride(0), out.data_ptr(), out.stride(0), R, HW, Cc, groups,
                                        gamma.data_ptr(), beta.data_ptr(), eps, int(silu), ws.data_ptr(),
                                        ws.numel() * 4, _DT[dt], _stream()), "iir_groupnorm_nhwc")
    return out


def layernorm(x, out, gamma=None, beta=None, eps=1e-5, shift=None, scale=None, rows_per_mod=1, transposed=False,
              tr_rows=1, tr_bstride=0):
    """`out` of dtype torch.float8_e4m3fn (or uint8): the normalised rows are stored as E4M3 bytes (rounded to fp16 first) -- the
    A operand of an all-fp8 GEMM (`gemm_fp8`)."""
    if x.dim() != 2 or out.dim() != 2:
        raise ValueError(f"layernorm: x and out are 2-D, got {tuple(x.shape)} and {tuple(out.shape)}")
    if transposed:
        need = (x.shape[0] - 1) // tr_rows * tr_bstride + (x.shape[0] - 1) % tr_rows + 1 if tr_rows > 0 else 0
        if tr_rows <= 0 or out.shape[0] != x.shape[1] or out.shape[1] < need:
            raise ValueError(f"layernorm: a transposed `out` is ({x.shape[1]}, >= {need}) with tr_rows > 0, got {tuple(out.shape)}")
    elif tuple(out.shape) != tuple(x.shape):
        raise ValueError(f"layernorm: out needs x's shape {tuple(x.shape)}, got {tuple(out.shape)}")
    _chk_cols("layernorm", x.shape[1], gamma=gamma, beta=beta, shift=shift, scale=scale)
    if (shift is None) != (scale is None) or (shift is not None and (rows_per_mod <= 0 or shift.dim() != 2 or scale.dim() != 2
                                                                      or scale.stride(0) != shift.stride(0)
                                                                      or shift.shape[0] * rows_per_mod < x.shape[0]
                                                                      or scale.shape[0] * rows_per_mod < x.shape[0])):
        raise ValueError("layernorm: shift and scale come together, 2-D with one row stride, a row per `rows_per_mod` rows of x")
    _chk2d(x, "x")
    if out.dtype in (torch.float8_e4m3fn, torch.uint8):
        if transposed or out.dim() != 2 or out.stride(1) != 1 or out.stride(0) % 8 or not out.is_cuda or out.shape != x.shape:
            raise ValueError("layernorm: an fp8 `out` needs x's shape, contiguous rows with a stride % 8 == 0, no transposition")
        transposed = 2
    else:
        _chk2d(out, "out")
    rows, Cc = x.shape
    ldmod = shift.stride(0) if shift is not None else 0
    L.check(L.load().iir_layernorm_f16(x.data_ptr(), x.stride(0), out.data_ptr(), out.stride(0), rows, Cc, _p(gamma),
                                       _p(beta), eps, _p(shift), _p(scale), ldmod, rows_per_mod, int(transposed), tr_rows,
                                       tr_bstride, _stream()), "iir_layernorm_f16")
    return out


def adaln_job_table(jobs, device):
    """jobs: list of (x, out, shift, scale, transposed) 2-D fp16 views -> device table of iir_adaln_job records.
    The caller keeps the views alive; the table holds raw addresses."""
    arr = (L.AdaLNJob * len(jobs))()
    for i, (x, out, shift, scale, tr) in enumerate(jobs):
        if x.dim() != 2 or out.dim() != 2:
            raise ValueError(f"adaln job {i}: x and out are 2-D, got {tuple(x.shape)} and {tuple(out.shape)}")
        rows, Cc = x.shape
        if Cc < 8 or Cc > 2560 or Cc % 8:       # ln_row walks 5 x 64 chunks of 8: a wider row would lose its tail silently
            raise ValueError(f"adaln job {i}: C must be a multiple of 8 in 8..2560, got {Cc}")
        if (out.shape[0] != Cc or out.shape[1] < rows) if tr else tuple(out.shape) != (rows, Cc):
            raise ValueError(f"adaln job {i}: out {tuple(out.shape)} does not fit x {tuple(x.shape)} (transposed: {bool(tr)})")
        _chk_cols(f"adaln job {i}", Cc, shift=shift, scale=scale)
        _chk2d(x, "x"); _chk2d(out, "out")
        arr[i] = L.AdaLNJob(x.data_ptr(), out.data_ptr(), shift.data_ptr(), scale.data_ptr(), x.stride(0), out.stride(0),
                            x.shape[1], int(tr))
    raw = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
    return raw.to(device)


def adaln_batch(table, njobs, rows, max_C, ldmod, rows_per_mod, tr_rows, tr_bstride, eps=1e-6):
    L.check(L.load().iir_adaln_batch_f16(table.data_ptr(), njobs, rows, max_C, eps, ldmod, rows_per_mod, tr_rows, tr_bstride,
                                         _stream()), "iir_adaln_batch_f16")


def _refuse(who, ok, msg):
    """The pointwise entries get pointers: what a launch would touch outside a tensor is refused here, before any library call."""
    if not ok:
        raise ValueError(f"{who}: {msg}")


def _image_source(who, t, name, unit=" in [0, 1]"):
    """An image batch as the image kernels read it -> (whether it is uint8 interleaved, (N, C, H, W))."""
    if not torch.is_tensor(t) or t.dim() != 4 or t.dtype not in (torch.float32, torch.uint8) or not t.is_contiguous():
        raise ValueError(f"{who}: {name} must be a contiguous 4-D tensor, fp32 (N, C, H, W){unit} or uint8 (N, H, W, C), got "
                         f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
    if t.dtype != torch.uint8:
        return False, tuple(t.shape)
    N, H, W, Cc = t.shape
    return True, (N, Cc, H, W)


def _workspace(who, ws, need, device, where="the images' device"):
    """The byte workspace of a launch: the caller's, checked against `need` bytes, or a fresh one when absent."""
    if ws is None:
        return torch.empty((need + 7) // 8, dtype=torch.float64, device=device)
    _refuse(who, torch.is_tensor(ws) and ws.is_cuda and ws.device == device and ws.is_contiguous()
            and ws.numel() * ws.element_size() >= need and ws.data_ptr() % 8 == 0,
            f"ws needs {need} contiguous, 8-byte aligned bytes on {where}")
    return ws


def _chk_rows2d(who, name, t, rows, cols):
    """2-D fp16 / bf16 view with unit column stride that holds `rows` x `cols` (exactly `rows` rows, at least `cols` columns)."""
    _refuse(who, t.dim() == 2 and t.dtype in _DT and t.stride(1) == 1 and t.shape[0] == rows and t.shape[1] >= cols,
            f"{name} must be a 2-D fp16 / bf16 view of {rows} rows and at least {cols} unit-stride columns, got {t.dtype} "
            f"{tuple(t.shape)} {t.stride()}")


def sinusoid(vals, out, dim, col_off=0):
    """vals fp32 (rows, n_vals) device tensor; out 2-D fp16 view."""
    _refuse("sinusoid", vals.dim() == 2 and vals.dtype == torch.float32 and vals.is_contiguous(),
            f"vals must be a contiguous 2-D fp32 tensor, got {vals.dtype} {tuple(vals.shape)} {vals.stride()}")
    rows, n_vals = vals.shape
    _refuse("sinusoid", out.dim() == 2 and out.dtype == torch.float16 and out.stride(1) == 1 and col_off >= 0 and out.shape[0] >= rows
            and out.shape[1] >= col_off + n_vals * dim,
            f"out must be a 2-D fp16 view of at least {rows} x ({col_off} + {n_vals} * {dim}), got {out.dtype} {tuple(out.shape)}")
    L.check(L.load().iir_sinusoid_f16(vals.data_ptr(), n_vals, rows, dim, out.data_ptr(), out.stride(0), col_off,
                                      _stream()), "iir_sinusoid_f16")
    return out


def silu(x, out):
    _refuse("silu", x.dtype == torch.float16 and out.dtype == torch.float16 and x.is_contiguous() and out.is_contiguous()
            and out.numel() == x.numel(),
            f"x and out must be contiguous fp16 tensors of one size, got {x.dtype} {tuple(x.shape)} and {out.dtype} {tuple(out.shape)}")
    L.check(L.load().iir_silu_f16(x.data_ptr(), out.data_ptr(), x.numel(), _stream()), "iir_silu_f16")
    return out


def copy_add(src, dst, dst_off=0, add=None, add_scale=None, rows_per_scale=1):
    """dst[:, dst_off:dst_off+C] = src + add * add_scale[row // rows_per_scale]."""
    _chk2d(src, "src"); _chk2d(dst, "dst")
    M, Cc = src.shape
    _refuse("copy_add", dst_off >= 0 and dst.shape[0] >= M and dst.shape[1] >= dst_off + Cc,
            f"dst {tuple(dst.shape)} does not hold {M} rows of {Cc} columns from column {dst_off}")
    if add is not None:
        _chk2d(add, "add")
        _refuse("copy_add", tuple(add.shape) == (M, Cc), f"add {tuple(add.shape)} must have src's shape {(M, Cc)}")
    if add_scale is not None:
        _refuse("copy_add", rows_per_scale > 0 and add_scale.dtype == torch.float32 and add_scale.is_contiguous()
                and add_scale.numel() >= -(-M // max(rows_per_scale, 1)),
                f"add_scale must be contiguous fp32 with a value per {rows_per_scale} of {M} rows, got {add_scale.dtype} {add_scale.numel()}")
    L.check(L.load().iir_copy_add_f16(src.data_ptr(), src.stride(0), dst.data_ptr(), dst.stride(0), dst_off, M, Cc,
                                      _p(add), add.stride(0) if add is not None else 0, _p(add_scale), rows_per_scale,
                                      _stream()), "iir_copy_add_f16")
    return dst


FREEU_SLABS = L.MACROS["IIR_FREEU_SLABS"]


def freeu_partials_floats(rows, H, W, C):
    """fp32 elements of the partials buffer freeu_stats leaves for a (rows, C) skip of H x W images."""
    n = L.load().iir_freeu_partials_bytes(rows, H, W, C)
    if n < 0:
        raise ValueError(f"freeu: invalid geometry rows={rows} H={H} W={W} C={C}")
    return n // 4


def freeu_stats(skip, partials, H, W, add=None, add_scale=None):
    """FreeU filter sums of t = skip + add * add_scale[row // (H*W)] per (image, channel, HW slab) into fp32 `partials`."""
    _chk2d(skip, "skip")
    M, Cc = skip.shape
    L.check(L.load().iir_freeu_stats_f16(skip.data_ptr(), skip.stride(0), _p(add), add.stride(0) if add is not None else 0,
                                         _p(add_scale), M, H, W, Cc, partials.data_ptr(), partials.numel() * 4, _stream()),
            "iir_freeu_stats_f16")
    return partials


def freeu_concat(x, skip, dst, partials, H, W, b, s, dst_off=0, mid_add=None, add=None, add_scale=None):
    """dst[:, dst_off:+cx] = (x + mid_add * add_scale), its first cx // 2 channels times b; dst[:, dst_off+cx:+cs] =
    fourier_filter(skip + add * add_scale, threshold 1, scale s) from the sums freeu_stats left in `partials`."""
    _chk2d(x, "x"); _chk2d(skip, "skip"); _chk2d(dst, "dst")
    M, cx = x.shape
    cs = skip.shape[1]
    if skip.shape[0] != M or dst.shape[0] != M:
        raise ValueError("freeu_concat: x, skip and dst must have the same rows")
    L.check(L.load().iir_freeu_concat_f16(x.data_ptr(), x.stride(0), cx, _p(mid_add), mid_add.stride(0) if mid_add is not None else 0,
                                          skip.data_ptr(), skip.stride(0), cs, _p(add), add.stride(0) if add is not None else 0,
                                          _p(add_scale), M, H, W, float(b), float(s), partials.data_ptr(), partials.numel() * 4,
                                          dst.data_ptr(), dst.stride(0), dst_off, _stream()), "iir_freeu_concat_f16")
    return dst


SEG_MAX_EXTENT = L.MACROS["IIR_SEG_MAX_EXTENT"]


def seg_blur_q(q, images, H, W, wy=None, wx=None, mean=False):
    """Smoothed-energy guidance: blur the (images * H * W, C) query view `q` (a column slice of the q | k buffer, starting at
    the first perturbed row) over the H x W token grid, in place: fp32 taps `wy` (along H) and `wx` (along W), reflect border;
    `mean`: every token becomes its image's mean instead (the taps are not read)."""
    _chk2d(q, "q")
    M, Cc = q.shape
    if M != images * H * W:
        raise ValueError(f"seg_blur_q: q has {M} rows, {images} images of {H} x {W} tokens need {images * H * W}")
    if not mean:
        for name, t in (("wy", wy), ("wx", wx)):
            if t is None or t.dtype != torch.float32 or t.dim() != 1 or not t.is_contiguous() or not t.is_cuda:
                raise ValueError(f"seg_blur_q: {name} must be a contiguous 1-D fp32 CUDA tensor")
    L.check(L.load().iir_seg_blur_q_f16(q.data_ptr(), q.stride(0), images, H, W, Cc, _p(wy), 0 if wy is None else wy.numel(),
                                        _p(wx), 0 if wx is None else wx.numel(), int(bool(mean)), _stream()), "iir_seg_blur_q_f16")
    return q


def pack_latent(x, out, rep=1, scale=1.0):
    """x fp32 (B,C,H,W) contiguous -> out 2-D fp16 view (rep*B*H*W, ld>=C).  `scale`: a float, or an fp32 CUDA tensor (one
    element) read at launch time (iir_pack_latent_dscale)."""
    B, Cc, H, Wd = x.shape
    assert x.dtype == torch.float32 and x.is_contiguous() and out.dtype in _DT
    _refuse("pack_latent", rep > 0, f"rep must be positive, got {rep}")
    _chk_rows2d("pack_latent", "out", out, rep * B * H * Wd, Cc)
    h, args = L.load(), (x.data_ptr(), B, Cc, H * Wd, out.data_ptr(), out.stride(0), rep)
    if torch.is_tensor(scale):
        assert scale.dtype == torch.float32 and scale.is_cuda and scale.numel() >= 1
        L.check(h.iir_pack_latent_dscale(*args, scale.data_ptr(), _DT[out.dtype], _stream()), "iir_pack_latent_dscale")
    else:
        L.check(h.iir_pack_latent_t(*args, scale, _DT[out.dtype], _stream()), "iir_pack_latent_t")
    return out


def unpack_latent(x2d, out):
    """x2d fp16 view (R*H*W, ld) -> out fp32 (R,C,H,W)."""
    R, Cc, H, Wd = out.shape
    assert out.dtype == torch.float32 and out.is_contiguous() and x2d.dtype in _DT
    _chk_rows2d("unpack_latent", "x2d", x2d, R * H * Wd, Cc)
    L.check(L.load().iir_unpack_latent_t(x2d.data_ptr(), x2d.stride(0), R, Cc, H * Wd, out.data_ptr(), _DT[x2d.dtype], _stream()),
            "iir_unpack_latent_t")
    return out


def _chk_pag(pag_scale):
    if not (torch.is_tensor(pag_scale) and pag_scale.is_cuda and pag_scale.dtype == torch.float32 and pag_scale.numel() >= 1):
        raise ValueError("pag_scale must be a CUDA fp32 tensor (the step's s_t, read at launch time)")


def _sched_desc(eps2d, B, coef, x, pag_scale, cfg=True):
    """A SchedDesc with the fields iir_cfg_rescale_factor and iir_sched_step share."""
    _, Cc, H, Wd = x.shape
    d = L.SchedDesc(eps_nhwc=eps2d.data_ptr(), lde=eps2d.stride(0), B=B, C=Cc, HW=H * Wd, cfg=int(cfg), coef=coef.data_ptr())
    if pag_scale is not None:
        _chk_pag(pag_scale)
        d.groups, d.pag_scale = L.STEP_PAG, pag_scale.data_ptr()
    return d


def _chk_group(what, items):
    for name, t, numel in items:
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == numel):
            raise ValueError(f"{what} {name} must be a contiguous CUDA fp32 tensor of {numel} elements")


def apg_workspace(B, device):
    """The partial-sum workspace of `apg_project` for B images (iir_apg_project_workspace_bytes)."""
    return torch.empty(int(L.load().iir_apg_project_workspace_bytes(int(B))) // 8, dtype=torch.float64, device=device)


def apg_project(eps2d, B, coef, x, apg, ws):
    """The per-image half of adaptive projected guidance (iir_apg_project).  `apg` = (avg (shape of x), sa (2B,), par
    {eta, r, beta_t, 0}), fp32 CUDA tensors: avg holds the running average A_prev and then A (never loaded when beta_t == 0),
    sa receives {s, alpha} per image.  `ws`: an `apg_workspace(B, device)`.  `coef` and `x` as for `sched_step`."""
    _, Cc, H, Wd = x.shape
    avg, sa, par = apg
    _chk_group("apg_project: apg", (("avg", avg, x.numel()), ("sa", sa, 2 * B), ("par", par, 4)))
    if not (torch.is_tensor(ws) and ws.is_cuda and ws.is_contiguous() and ws.dtype == torch.float64):
        raise ValueError("apg_project: ws must be a contiguous CUDA fp64 tensor (ops.apg_workspace)")
    L.check(L.load().iir_apg_project(eps2d.data_ptr(), eps2d.stride(0), B, Cc, H * Wd, coef.data_ptr(), x.data_ptr(), par.data_ptr(),
                                     avg.data_ptr(), sa.data_ptr(), ws.data_ptr(), ws.numel() * 8, _stream()), "iir_apg_project")
    return sa


def sched_step(eps2d, B, coef, x, prev, noise=None, cfg=True, x0_out=None, eps_out=None, eps_factor=None, pag_scale=None, hist=None,
               keep=None, apg=None):
    """One iir_sched_step call; each optional group sets its IIR_STEP_* bit in the descriptor.
    `pag_scale` (device fp32[1]): the PAG form -- eps2d holds the perturbed rows after the cond rows (IIR_STEP_PAG).
    `hist` (shape of x, fp32): adds the history term coef[7] * hist and then holds this step's x0 (IIR_STEP_HIST).
    `keep` = (map (B, H*W), src, noise0, coef {thr, a, b, 0}), fp32 CUDA tensors: the restore-map form (IIR_STEP_KEEP) --
    pixels with map <= thr store a * src + b * noise0 in prev instead of the update.
    `apg` = (avg, sa, par), as `apg_project` left them: the guided eps is the projected form (IIR_STEP_APG); it needs `cfg`
    and does not combine with `eps_factor` (the norm clamp is APG's answer to what rescale_noise_cfg addresses)."""
    if apg is not None and eps_factor is not None:
        raise ValueError("sched_step: apg is not available together with eps_factor")
    if apg is not None and not cfg:
        raise ValueError("sched_step: apg needs cfg (there is nothing to project without the uncond rows)")
    d = _sched_desc(eps2d, B, coef, x, pag_scale, cfg)
    d.x, d.noise, d.prev = x.data_ptr(), _p(noise), prev.data_ptr()
    d.x0_out, d.eps_out, d.eps_factor = _p(x0_out), _p(eps_out), _p(eps_factor)
    if hist is not None:
        assert hist.shape == x.shape and hist.dtype == torch.float32 and hist.is_contiguous()
        if eps_out is not None:
            raise ValueError("sched_step: eps_out is not available together with hist")
        d.groups |= L.STEP_HIST
        d.hist = hist.data_ptr()
    if keep is not None:
        n = x.numel()
        _chk_group("sched_step: keep", zip(("map", "src", "noise", "coef"), keep, (B * d.HW, n, n, 4)))
        d.groups |= L.STEP_KEEP
        d.keep_map, d.keep_src, d.keep_noise, d.keep_coef = [t.data_ptr() for t in keep]
    if apg is not None:
        _chk_group("sched_step: apg", zip(("avg", "sa", "par"), apg, (x.numel(), 2 * B, 4)))
        d.groups |= L.STEP_APG
        d.apg_avg, d.apg_sa, d.apg_par = [t.data_ptr() for t in apg]
    L.check(L.load().iir_sched_step(C.byref(d), _stream()), "iir_sched_step")
    return prev


def cfg_rescale_factor(eps2d, B, coef, x, guidance_rescale, factor, pag_scale=None):
    """factor (B,) fp32 device: the per-image multiplier `rescale_noise_cfg` applies to the guided eps (with `pag_scale`: the
    guided eps includes the PAG term of rows [2B, 3B))."""
    d = _sched_desc(eps2d, B, coef, x, pag_scale)
    L.check(L.load().iir_cfg_rescale_factor(C.byref(d), float(guidance_rescale), factor.data_ptr(), _stream()), "iir_cfg_rescale_factor")
    return factor


def segment_job_table(jobs, device):
    """Device int64 (n, 3) table for `copy_segments` from (src, dst) pairs of equal-size contiguous tensors.  Returns
    (table, n, max_units)."""
    rows = []
    for src, dst in jobs:
        nb = src.numel() * src.element_size()
        if (not src.is_contiguous() or not dst.is_contiguous() or dst.numel() * dst.element_size() != nb or nb % 16
                or src.data_ptr() % 16 or dst.data_ptr() % 16):
            raise ValueError("copy_segments: each job needs contiguous, 16-byte aligned tensors of the same size (a multiple of 16 B)")
        rows.append([src.data_ptr(), dst.data_ptr(), nb // 16])
    table = torch.tensor(rows, dtype=torch.int64).to(device)
    return table, len(rows), max(r[2] for r in rows)


def copy_segments(table, njobs, max_units):
    """Every job of a `segment_job_table` in one launch (iir_copy_segments)."""
    L.check(L.load().iir_copy_segments(table.data_ptr(), int(njobs), int(max_units), _stream()), "iir_copy_segments")


def lcm_step(eps2d, B, rep, coef, x, out2d, out_nchw=None):
    _, Cc, H, Wd = x.shape
    _refuse("lcm_step", B > 0 and rep > 0 and x.dtype == torch.float32 and x.is_contiguous() and x.shape[0] == B,
            f"x must be contiguous fp32 ({B}, C, H, W) with rep > 0, got {x.dtype} {tuple(x.shape)}, rep {rep}")
    for name, t2 in (("eps2d", eps2d), ("out2d", out2d)):
        _refuse("lcm_step", t2.dtype == torch.float16, f"{name} must be fp16, got {t2.dtype}")
        _chk_rows2d("lcm_step", name, t2, rep * B * H * Wd, Cc)
    if out_nchw is not None:
        _refuse("lcm_step", out_nchw.dtype == torch.float32 and out_nchw.is_contiguous() and tuple(out_nchw.shape) == (rep * B, Cc, H, Wd),
                f"out_nchw must be contiguous fp32 {(rep * B, Cc, H, Wd)}, got {out_nchw.dtype} {tuple(out_nchw.shape)}")
    L.check(L.load().iir_lcm_step(eps2d.data_ptr(), eps2d.stride(0), B, rep, Cc, H * Wd, coef.data_ptr(), x.data_ptr(),
                                  out2d.data_ptr(), out2d.stride(0), _p(out_nchw), _stream()), "iir_lcm_step")
    return out2d


def transpose(x, out, rows_pad):
    _chk2d(x, "x"); _chk2d(out, "out")
    rows, cols = x.shape
    _refuse("transpose", out.shape[0] >= cols and out.shape[1] >= rows_pad >= rows,
            f"out {tuple(out.shape)} does not hold {cols} rows of rows_pad = {rows_pad} >= {rows} columns")
    L.check(L.load().iir_transpose_f16(x.data_ptr(), x.stride(0), rows, cols, out.data_ptr(), out.stride(0), rows_pad,
                                       _stream()), "iir_transpose_f16")
    return out


def sched_step_f32(eps, x, coef, prev, noise=None, x0_out=None, hist=None):
    """fp32 contiguous tensors of equal shape; coef fp32 device (8,).  `hist`: the history term, k_h in coef[7], as in sched_step."""
    name, hp = ("iir_sched_step_f32", []) if hist is None else ("iir_sched_step_hist_f32", [hist.data_ptr()])
    L.check(getattr(L.load(), name)(eps.data_ptr(), x.data_ptr(), _p(noise), coef.data_ptr(), *hp, x.numel(), prev.data_ptr(),
                                    _p(x0_out), _stream()), name)
    return prev


# The earlier spellings of the hist / device-scale forms: the GPU tests call them, and so may code outside the package.
def sched_step_hist(eps2d, B, coef, x, hist, prev, **kw):
    return sched_step(eps2d, B, coef, x, prev, hist=hist, **kw)


def sched_step_hist_f32(eps, x, coef, hist, prev, **kw):
    return sched_step_f32(eps, x, coef, prev, hist=hist, **kw)


def pack_latent_dscale(x, out, scale, rep=1):
    return pack_latent(x, out, rep=rep, scale=scale)


def axpby_f32(x, y, coef, out):
    L.check(L.load().iir_axpby_f32(x.data_ptr(), y.data_ptr(), coef.data_ptr(), x.numel(), out.data_ptr(), _stream()),
            "iir_axpby_f32")
    return out


def prefetch(ptr, nbytes, blocks=32):
    """Pull [ptr, ptr+nbytes) towards the Infinity Cache on the current stream."""
    L.check(L.load().iir_prefetch(ptr, nbytes, blocks, _stream()), "iir_prefetch")


def softmax_rows(x):
    """In-place softmax over the columns of a 2-D fp16 view (cols <= 16384)."""
    _chk2d(x, "x")
    L.check(L.load().iir_softmax_rows_f16(x.data_ptr(), x.stride(0), x.shape[0], x.shape[1], _stream()), "iir_softmax_rows_f16")
    return x


def softmax_rows_f32(s, p):
    """p = softmax over the columns of the fp32 scores s (cols <= 16384, % 4 == 0); p is fp16 or bf16."""
    if (s.dtype != torch.float32 or s.dim() != 2 or s.stride(1) != 1 or p.dtype not in _DT or p.shape != s.shape or p.stride(1) != 1
            or not (s.is_cuda and p.is_cuda)):
        raise ValueError("softmax_rows_f32: s fp32 2-D, p fp16/bf16 of the same shape, both on the GPU with unit column stride")
    L.check(L.load().iir_softmax_rows_f32(s.data_ptr(), s.stride(0), p.data_ptr(), p.stride(0), s.shape[0], s.shape[1], _DT[p.dtype],
                                          _stream()), "iir_softmax_rows_f32")
    return p


def blend_tiles(a, b, extent, vertical):
    """In-place seam blend of fp32 NCHW tile `b` with its upper (vertical) or left neighbour `a`."""
    assert a.dtype == b.dtype == torch.float32 and a.is_contiguous() and b.is_contiguous()
    _refuse("blend_tiles", a.dim() == 4 and b.dim() == 4 and a.shape[0] * a.shape[1] == b.shape[0] * b.shape[1],
            f"a {tuple(a.shape)} and b {tuple(b.shape)} must be 4-D with equal plane counts")
    L.check(L.load().iir_blend_tiles_f32(a.data_ptr(), b.data_ptr(), a.shape[0] * a.shape[1], a.shape[2], a.shape[3], b.shape[2],
                                         b.shape[3], extent, int(vertical), _stream()), "iir_blend_tiles_f32")
    return b


COLOR_FIX_MODES = ("wavelet", "adain")
MAX_MAP_FEATHER = L.MACROS["IIR_REGION_MAX_FEATHER"]


def colorfix(content, style, mode, out=None, ws=None):
    """LQ-guided colour correction (DESIGN.md section 7 "Colour fix"): content, style fp32 (B, C, H, W) in [0, 1], contiguous,
    on the same device; mode "wavelet" or "adain".  `out` may be `content` (in place); `ws` a byte workspace of at least
    iir_colorfix_workspace_bytes (allocated here when absent)."""
    if mode not in COLOR_FIX_MODES:
        raise ValueError(f"colorfix: mode must be one of {COLOR_FIX_MODES}, got {mode!r}")
    for name, t in (("content", content), ("style", style)):
        if t.dtype != torch.float32 or t.dim() != 4 or not t.is_contiguous() or not t.is_cuda:
            raise ValueError(f"colorfix: {name} must be a contiguous 4-D fp32 CUDA tensor, got {t.dtype} {tuple(t.shape)} {t.stride()}")
    if style.shape != content.shape or style.device != content.device:
        raise ValueError(f"colorfix: style {tuple(style.shape)} on {style.device} does not match content {tuple(content.shape)} on {content.device}")
    if out is None:
        out = torch.empty_like(content)
    elif out.dtype != torch.float32 or out.shape != content.shape or not out.is_contiguous() or out.device != content.device:
        raise ValueError("colorfix: out must be a contiguous fp32 tensor of content's shape on its device")
    B, Cc, H, W = content.shape
    if mode == "adain" and H * W < 2:
        raise ValueError("colorfix: adain needs at least 2 pixels per plane (unbiased variance)")
    h = L.load()
    need = h.iir_colorfix_workspace_bytes(B, Cc, H, W)
    if need < 0:
        raise ValueError(f"colorfix: unsupported geometry B={B} C={Cc} H={H} W={W}")
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device=content.device)
    elif not ws.is_cuda or not ws.is_contiguous() or ws.numel() * ws.element_size() < need:
        raise ValueError(f"colorfix: workspace needs {need} contiguous bytes on the device")
    fn = h.iir_colorfix_wavelet_f32 if mode == "wavelet" else h.iir_colorfix_adain_f32
    L.check(fn(content.data_ptr(), style.data_ptr(), out.data_ptr(), B, Cc, H, W, ws.data_ptr(), ws.numel() * ws.element_size(),
               _stream()), f"iir_colorfix_{mode}_f32")
    return out


def _chk_f32(t, name, dim):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == dim and t.is_contiguous()):
        raise ValueError(f"{name} must be a contiguous {dim}-D fp32 CUDA tensor")


def map_pool_max(map_px, factor, out=None):
    """Restore map at latent resolution: map_px fp32 (B, H, W) -> (B, H / factor, W / factor), the maximum over each
    factor x factor block (iir_map_pool_max_f32).  H and W must be multiples of `factor`."""
    _chk_f32(map_px, "map_pool_max: map_px", 3)
    B, H, W = map_px.shape
    if factor <= 0 or H % factor or W % factor:
        raise ValueError(f"map_pool_max: {H}x{W} is not a multiple of the factor {factor}")
    if out is None:
        out = torch.empty(B, H // factor, W // factor, dtype=torch.float32, device=map_px.device)
    else:
        _chk_f32(out, "map_pool_max: out", 3)
        if tuple(out.shape) != (B, H // factor, W // factor) or out.device != map_px.device:
            raise ValueError("map_pool_max: out must be (B, H / factor, W / factor) on the map's device")
    L.check(L.load().iir_map_pool_max_f32(map_px.data_ptr(), B, H, W, int(factor), out.data_ptr(), _stream()), "iir_map_pool_max_f32")
    return out


def region_composite(decoded, original, map_px, feather, out=None, ws=None):
    """Pixel composite under a restore map (DESIGN.md section 7 "Restore map"): decoded, original fp32 (B, C, H, W), map_px
    fp32 (B, H, W); `feather` = r, the half width of the box window in pixels (0: hard paste).  `out` may be `decoded` (in
    place); `ws`: a byte workspace of at least iir_region_composite_workspace_bytes (allocated here when absent)."""
    _chk_f32(decoded, "region_composite: decoded", 4)
    _chk_f32(original, "region_composite: original", 4)
    _chk_f32(map_px, "region_composite: map_px", 3)
    B, Cc, H, W = decoded.shape
    if original.shape != decoded.shape or tuple(map_px.shape) != (B, H, W) or original.device != decoded.device or map_px.device != decoded.device:
        raise ValueError(f"region_composite: original {tuple(original.shape)} / map {tuple(map_px.shape)} do not match decoded "
                         f"{tuple(decoded.shape)} on {decoded.device}")
    h = L.load()
    r = int(feather)
    if r < 0 or r > MAX_MAP_FEATHER:
        raise ValueError(f"region_composite: feather must be in [0, {MAX_MAP_FEATHER}], got {feather}")
    if out is None:
        out = torch.empty_like(decoded)
    else:
        _chk_f32(out, "region_composite: out", 4)
        if out.shape != decoded.shape or out.device != decoded.device:
            raise ValueError("region_composite: out must have decoded's shape and device")
    need = h.iir_region_composite_workspace_bytes(B, H, W)
    if need < 0:
        raise ValueError(f"region_composite: unsupported geometry B={B} H={H} W={W}")
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device=decoded.device)
    elif not ws.is_cuda or not ws.is_contiguous() or ws.numel() * ws.element_size() < need:
        raise ValueError(f"region_composite: workspace needs {need} contiguous bytes on the device")
    L.check(h.iir_region_composite_f32(decoded.data_ptr(), original.data_ptr(), map_px.data_ptr(), B, Cc, H, W, r, ws.data_ptr(),
                                       ws.numel() * ws.element_size(), out.data_ptr(), _stream()), "iir_region_composite_f32")
    return out


LQ_FIDELITY_MAX_RADIUS = L.MACROS["IIR_LQ_FIDELITY_MAX_RADIUS"]
LQ_FIDELITY_TILE = L.MACROS["IIR_LQ_FIDELITY_TILE"]           # the output tile a workgroup owns, per axis


def lq_fidelity(x0, lq, wc, prev, x0_out, taps=None, hist=None):
    """LQ fidelity guidance behind a scheduler step (iir_lq_fidelity_f32; DESIGN.md section 7 "LQ fidelity"): with
    delta = w * LP(lq - x0), x0_out = x0 + delta, prev += c * delta (in place) and, when given, hist = x0_out.  x0, lq, prev,
    x0_out, hist: fp32 (B, C, H, W) of one shape, each a tensor of its own (x0_out may not be x0: neighbouring tiles read x0);
    `wc`: fp32 CUDA {w, c}, read at launch time; `taps`: the 2 r + 1 normalised fp32 Gaussian taps of LP on the device, None
    for r = 0 (LP = identity, no filter arithmetic)."""
    _chk_f32(x0, "lq_fidelity: x0", 4)
    n = x0.numel()
    _chk_group("lq_fidelity:", (("lq", lq, n), ("prev", prev, n), ("x0_out", x0_out, n), ("wc", wc, 2))
               + ((("hist", hist, n),) if hist is not None else ()))
    r = 0
    if taps is not None:
        _chk_f32(taps, "lq_fidelity: taps", 1)
        if taps.numel() % 2 != 1 or taps.numel() // 2 > LQ_FIDELITY_MAX_RADIUS:
            raise ValueError(f"lq_fidelity: taps must hold 2 r + 1 values with r <= {LQ_FIDELITY_MAX_RADIUS}, got {taps.numel()}")
        r = taps.numel() // 2
    B, Cc, H, W = x0.shape
    L.check(L.load().iir_lq_fidelity_f32(x0.data_ptr(), lq.data_ptr(), _p(taps) if r else None, r, wc.data_ptr(), B * Cc, H, W,
                                         prev.data_ptr(), x0_out.data_ptr(), _p(hist), _stream()), "iir_lq_fidelity_f32")
    return x0_out


def _resample_pass(src, u8, dst, dims, axis, out_size, tables, win, quantize, clamp, scale, bias):
    bounds, weights, ksize = tables
    d = L.ResampleDesc()
    d.src, d.src_u8, d.dst = src.data_ptr(), int(u8), dst.data_ptr()
    d.N, d.C, d.H, d.W = dims
    d.axis, d.out_size = axis, out_size
    d.bounds, d.weights, d.ksize = bounds.data_ptr(), weights.data_ptr(), ksize
    d.y0, d.x0, d.h, d.w = win
    d.quantize, d.clamp = int(quantize), int(clamp is not None)
    d.lo, d.hi = clamp if clamp is not None else (0.0, 0.0)
    d.scale, d.bias = _p(scale), _p(bias)
    L.check(L.load().iir_resample_pass(C.byref(d), _stream()), "iir_resample_pass")


def resample(src, size, filter="bilinear", quantize=False, window=None, clamp=None, scale=None, bias=None, out=None):
    """Antialiased resize with PIL's filter definitions (iir_resample_pass; DESIGN.md section 7 "Resampling").  `src`: a
    contiguous CUDA tensor, fp32 planar (N, C, H, W) or uint8 interleaved (N, H, W, C) (0..255 units are kept); `size` =
    (H, W) of the full output; `filter` one of resample.FILTERS.  The horizontal pass runs first, then the vertical one, an
    axis that keeps its size is skipped, and equal sizes with no option are a plain copy.
    `quantize`: every pass ends in floor(v + 0.5) clamped to [0, 255] -- PIL's arithmetic on an 8-bit image.
    `window` = (y0, x0, h, w): only that part of the output is computed and returned.
    `clamp` = (lo, hi), then `scale` / `bias` (a number, one per channel, or an fp32 tensor of C): v * scale[c] + bias[c],
    both on the last pass.  Returns fp32 (N, C, h, w) (`out` when given; it may not overlap `src`)."""
    from . import resample as RS
    (oh, ow), win, clamp = RS.check_args(size, filter, quantize, window, clamp)
    u8, (N, Cc, H, W) = _image_source("resample", src, "src", unit="")
    if min(N, Cc, H, W) <= 0 or H > RS.MAX_SIDE or W > RS.MAX_SIDE or N * Cc > RS.MAX_PLANES:
        raise ValueError(f"resample: unsupported geometry N={N} C={Cc} H={H} W={W} (sides <= {RS.MAX_SIDE}, N * C <= {RS.MAX_PLANES})")
    y0, x0, h, w = win
    if out is not None:
        if not torch.is_tensor(out) or out.dtype != torch.float32 or tuple(out.shape) != (N, Cc, h, w) or not out.is_contiguous() \
                or out.device != src.device:
            raise ValueError(f"resample: out must be a contiguous fp32 tensor of shape {(N, Cc, h, w)} on src's device")
        lo_s, lo_o = src.data_ptr(), out.data_ptr()
        if lo_s < lo_o + out.numel() * 4 and lo_o < lo_s + src.numel() * src.element_size():
            raise ValueError("resample: out overlaps src")
    if not src.is_cuda:
        raise ValueError("resample: src must be a CUDA tensor (there is no host path)")
    dev = src.device
    scale, bias = RS.channel_vector(scale, Cc, dev, "scale"), RS.channel_vector(bias, Cc, dev, "bias")
    if out is None:
        out = torch.empty(N, Cc, h, w, dtype=torch.float32, device=dev)
    last = (quantize, clamp, scale, bias)
    if (oh, ow) == (H, W):
        if not u8 and window is None and not quantize and clamp is None and scale is None and bias is None:
            return out.copy_(src)
        _resample_pass(src, u8, out, (N, Cc, H, W), 0, W, RS.device_tables(W, W, None, dev), win, *last)
    elif oh == H:
        _resample_pass(src, u8, out, (N, Cc, H, W), 0, ow, RS.device_tables(W, ow, filter, dev), win, *last)
    elif ow == W:
        _resample_pass(src, u8, out, (N, Cc, H, W), 1, oh, RS.device_tables(H, oh, filter, dev), win, *last)
    else:
        mid = torch.empty(N, Cc, H, w, dtype=torch.float32, device=dev)          # the window's columns of every source row
        _resample_pass(src, u8, mid, (N, Cc, H, W), 0, ow, RS.device_tables(W, ow, filter, dev), (0, x0, H, w), quantize, None, None, None)
        _resample_pass(mid, False, out, (N, Cc, H, w), 1, oh, RS.device_tables(H, oh, filter, dev), (y0, 0, h, w), *last)
    return out


METRICS = ("psnr", "ssim")
METRICS_WINDOW = 11            # the SSIM window per axis: a cropped side below it has no SSIM
METRICS_TILE = L.MACROS["IIR_METRICS_TILE"]       # the SSIM-map tile a workgroup owns, per axis


def image_metrics(a, b, crop_border=0, y_channel=False, quantize=(False, False), what=("psnr", "ssim"), ws=None):
    """Per-image MSE and SSIM of two image batches (iir_image_metrics; DESIGN.md section 7 "Image metrics").  `a`, `b`:
    contiguous CUDA tensors of one device and one logical shape, each fp32 planar (N, C, H, W) on a [0, 1] scale or uint8
    interleaved (N, H, W, C), C 1 or 3; the arithmetic is in 0..255 units.  `crop_border`: pixels dropped on every side first;
    `y_channel` (C = 3): score the BT.601 luma alone; `quantize` = (for a, for b): an fp32 source is first rounded to the 8-bit
    image that would be saved; `what`: "psnr", "ssim" or both (a name or a sequence of names).  Returns fp64 (N, 2) =
    {MSE, SSIM} on the device; a column that `what` leaves out holds NaN.  PSNR = 10 log10(255^2 / MSE) is the caller's
    (instantir_amd.metrics).  `ws`: a byte workspace of at least iir_image_metrics_workspace_bytes (allocated here when absent)."""
    names = (what,) if isinstance(what, str) else tuple(what)
    if not names or any(w not in METRICS for w in names):
        raise ValueError(f"image_metrics: what must name one or both of {METRICS}, got {what!r}")
    a_u8, dims = _image_source("image_metrics", a, "a")
    b_u8, dims_b = _image_source("image_metrics", b, "b")
    if dims_b != dims:
        raise ValueError(f"image_metrics: b is (N, C, H, W) = {dims_b} but a is {dims}")
    N, Cc, H, W = dims
    if Cc not in (1, 3):
        raise ValueError(f"image_metrics: a and b must have 1 or 3 channels, got {Cc}")
    if y_channel and Cc != 3:
        raise ValueError("image_metrics: y_channel needs 3 channels")
    check_crop("image_metrics", crop_border)
    try:
        qa, qb = (bool(q) for q in quantize)
    except (TypeError, ValueError):
        raise ValueError(f"image_metrics: quantize must be a pair of flags (for a, for b), got {quantize!r}") from None
    need_side = METRICS_WINDOW if "ssim" in names else 1
    if min(N, H, W) <= 0 or min(H, W) - 2 * crop_border < need_side:
        raise ValueError(f"image_metrics: {H}x{W} with crop_border {crop_border} leaves less than {need_side} pixel(s) per side"
                         + (" (the SSIM window is 11 x 11)" if "ssim" in names else ""))
    if not a.is_cuda or not b.is_cuda or a.device != b.device:
        raise ValueError(f"image_metrics: a and b must be CUDA tensors on one device (there is no host path), got {a.device} and {b.device}")
    d = L.MetricsDesc()
    d.a, d.b, d.a_u8, d.b_u8 = a.data_ptr(), b.data_ptr(), int(a_u8), int(b_u8)
    d.a_quantize, d.b_quantize = int(qa), int(qb)
    d.N, d.C, d.H, d.W = N, Cc, H, W
    d.crop_border, d.y_channel = crop_border, int(bool(y_channel))
    d.what = (L.METRIC_PSNR if "psnr" in names else 0) | (L.METRIC_SSIM if "ssim" in names else 0)
    h = L.load()
    need = h.iir_image_metrics_workspace_bytes(C.byref(d))
    if need < 0:
        raise ValueError(f"image_metrics: unsupported geometry N={N} C={Cc} H={H} W={W} crop_border={crop_border}")
    ws = _workspace("image_metrics", ws, need, a.device)
    out = torch.empty(N, 2, dtype=torch.float64, device=a.device)
    d.ws, d.ws_bytes, d.out = ws.data_ptr(), ws.numel() * ws.element_size(), out.data_ptr()
    L.check(h.iir_image_metrics(C.byref(d), _stream()), "iir_image_metrics")
    return out


NIQE_BLOCK, NIQE_STATS = L.MACROS["IIR_NIQE_BLOCK"], L.MACROS["IIR_NIQE_STATS"]


def niqe_stats(src, crop_border=0, ws=None):
    """NIQE's per-block signed moments of a batch of images at two scales (iir_niqe_stats; DESIGN.md section 7 "NIQE").  `src`:
    a contiguous CUDA tensor, fp32 planar (N, C, H, W) on a [0, 1] scale or uint8 interleaved (N, H, W, C), C 1 or 3 (3 is scored
    on its BT.601 luma); `crop_border`: pixels dropped on every side first.  Returns fp64 (N, 2, nb, 26) on the device: per
    scale and 96 x 96 block (48 x 48 at scale 2) in raster order, five statistics of each of the five maps and the sum of sigma;
    `instantir_amd.niqe.features` takes it from there.  Fewer than two blocks is refused: the score needs a covariance.
    `ws`: a byte workspace of at least iir_niqe_workspace_bytes (allocated here when absent)."""
    u8, (N, Cc, H, W) = _image_source("niqe_stats", src, "src")
    if Cc not in (1, 3):
        raise ValueError(f"niqe_stats: src must have 1 or 3 channels, got {Cc}")
    check_crop("niqe_stats", crop_border)
    nbh, nbw = max(H - 2 * crop_border, 0) // NIQE_BLOCK, max(W - 2 * crop_border, 0) // NIQE_BLOCK
    if N <= 0 or nbh * nbw < 2:
        raise ValueError(f"niqe_stats: {H}x{W} with crop_border {crop_border} holds {nbh * nbw} block(s) of {NIQE_BLOCK} x {NIQE_BLOCK}; "
                         "NIQE needs at least two")
    if not src.is_cuda:
        raise ValueError(f"niqe_stats: src must be a CUDA tensor (there is no host path), got {src.device}")
    h = L.load()
    need = h.iir_niqe_workspace_bytes(N, Cc, H, W, crop_border)
    if need < 0:
        raise ValueError(f"niqe_stats: unsupported geometry N={N} C={Cc} H={H} W={W} crop_border={crop_border}")
    ws = _workspace("niqe_stats", ws, need, src.device)
    out = torch.empty(N, 2, nbh * nbw, NIQE_STATS, dtype=torch.float64, device=src.device)
    L.check(h.iir_niqe_stats(src.data_ptr(), int(u8), N, Cc, H, W, crop_border, ws.data_ptr(), ws.numel() * ws.element_size(),
                             out.data_ptr(), out.numel() * 8, _stream()), "iir_niqe_stats")
    return out


FILTER2D_MAX_KSIZE = L.MACROS["IIR_FILTER2D_MAX_KSIZE"]
JPEG_QUALITY_RANGE = (1.0, 99.0)


def _chk_image(who, t, name="x"):
    if not (torch.is_tensor(t) and t.dtype == torch.float32 and t.dim() == 4 and t.is_contiguous()) or min(t.shape) <= 0:
        raise ValueError(f"{who}: {name} must be a contiguous, non-empty fp32 (N, C, H, W) tensor, got "
                         f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")


def _chk_image_out(who, x, out, in_place):
    """`out` for an image launch: x's shape and device; the same tensor as x only where `in_place`, never a shifted view."""
    if out is None:
        return torch.empty_like(x)
    _chk_image(who, out, "out")
    if out.shape != x.shape or out.device != x.device:
        raise ValueError(f"{who}: out must have x's shape and device")
    lo_x, lo_o, nbytes = x.data_ptr(), out.data_ptr(), x.numel() * 4
    if lo_x < lo_o + nbytes and lo_o < lo_x + nbytes and not (in_place and lo_x == lo_o):
        raise ValueError(f"{who}: out overlaps x" + ("" if in_place else " (neighbouring tiles read x: it cannot run in place)"))
    return out


def _per_image(who, name, value, N, lo, hi, device):
    """A per-image launch parameter as fp32 (N,) on `device`: a number for every image, N numbers, or a tensor of N values
    (checked on the host: a device tensor is read back); every value finite and in [lo, hi]."""
    if torch.is_tensor(value):
        vals = value.detach().to("cpu", torch.float64).reshape(-1)
    else:
        try:
            vals = torch.tensor([float(value)] * N if isinstance(value, (int, float)) else [float(v) for v in value], dtype=torch.float64)
        except (TypeError, ValueError):
            raise ValueError(f"{who}: {name} must be a number or one number per image, got {value!r}") from None
    if vals.numel() != N:
        raise ValueError(f"{who}: {name} must hold one value per image ({N}), got {vals.numel()}")
    if not bool(((vals >= lo) & (vals <= hi)).all()):
        raise ValueError(f"{who}: {name} must lie in [{lo:g}, {hi:g}], got {vals.tolist()}")
    return vals.to(torch.float32).to(device)


def _chk_cuda(who, *tensors):
    if any(not t.is_cuda for t in tensors) or len({t.device for t in tensors}) != 1:
        raise ValueError(f"{who}: the tensors must be CUDA tensors on one device (there is no host path), got "
                         f"{[str(t.device) for t in tensors]}")


def filter2d(x, taps, out=None):
    """Per-image k x k blur with reflect padding (iir_filter2d_f32; DESIGN.md section 7 "Synthetic degradation"): x fp32
    (N, C, H, W); taps fp32 (N, k, k) or (k, k) for every image, k odd, <= 21, H and W > (k - 1) / 2.  `out` may not be x."""
    who = "filter2d"
    _chk_image(who, x)
    N, Cc, H, W = x.shape
    if not (torch.is_tensor(taps) and taps.dtype == torch.float32 and taps.dim() in (2, 3)):
        raise ValueError(f"{who}: taps must be an fp32 (N, k, k) or (k, k) tensor, got {getattr(taps, 'dtype', type(taps))} "
                         f"{tuple(getattr(taps, 'shape', ()))}")
    if taps.dim() == 2:
        taps = taps.unsqueeze(0).expand(N, -1, -1)
    k = taps.shape[-1]
    if taps.shape[0] != N or taps.shape[1] != k or k % 2 != 1 or k > FILTER2D_MAX_KSIZE:
        raise ValueError(f"{who}: taps must be ({N}, k, k) with k odd and <= {FILTER2D_MAX_KSIZE}, got {tuple(taps.shape)}")
    if min(H, W) <= (k - 1) // 2:
        raise ValueError(f"{who}: a {k} x {k} kernel needs H, W > {(k - 1) // 2} (one reflection), got {H}x{W}")
    if H > 32768 or W > 32768 or N * Cc > 65535:
        raise ValueError(f"{who}: unsupported geometry N={N} C={Cc} H={H} W={W} (sides <= 32768, N * C <= 65535)")
    out = _chk_image_out(who, x, out, in_place=False)
    _chk_cuda(who, x, taps, out)
    taps = taps.contiguous()
    L.check(L.load().iir_filter2d_f32(x.data_ptr(), taps.data_ptr(), N, Cc, H, W, k, out.data_ptr(), _stream()), "iir_filter2d_f32")
    return out


def add_gaussian_noise(x, sigma, seed, stream=0, gray=False, out=None):
    """out = clamp(x + (sigma[n] / 255) z, 0, 1) with z ~ N(0, 1) a pure function of (seed, stream, n, c, y, x) through
    Philox4x32-10 (iir_add_gaussian_noise_f32; DESIGN.md section 7 "Synthetic degradation").  x fp32 (N, C, H, W); `sigma`: a
    number or one per image, in 0..255 units, in [0, 255]; `seed` an integer in [0, 2^64); `stream` in [0, 2^32): stages of one
    recipe take different streams; `gray`: one z per pixel for all channels.  `out` may be x."""
    who = "add_gaussian_noise"
    _chk_image(who, x)
    N, Cc, H, W = x.shape
    for name, v, top in (("seed", seed, 1 << 64), ("stream", stream, 1 << 32)):
        if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v < top:
            raise ValueError(f"{who}: {name} must be an integer in [0, 2^{top.bit_length() - 1}), got {v!r}")
    if H * W >= 1 << 32 or (x.numel() + 255) // 256 > 0x7fffffff:
        raise ValueError(f"{who}: unsupported geometry N={N} C={Cc} H={H} W={W}")
    out = _chk_image_out(who, x, out, in_place=True)
    sig = _per_image(who, "sigma", sigma, N, 0.0, 255.0, "cpu")
    _chk_cuda(who, x, out)
    sig = sig.to(x.device)
    L.check(L.load().iir_add_gaussian_noise_f32(x.data_ptr(), sig.data_ptr(), N, Cc, H, W, seed, stream, int(bool(gray)), out.data_ptr(),
                                                _stream()), "iir_add_gaussian_noise_f32")
    return out


def jpeg_roundtrip(x, quality, out=None):
    """What a baseline 4:2:0 JPEG encode + decode at `quality` does to x, without entropy coding (iir_jpeg_roundtrip_f32;
    DESIGN.md section 7 "Synthetic degradation").  x fp32 (N, 3, H, W) in [0, 1]; `quality`: a number or one per image, in
    [1, 99].  `out` may be x."""
    who = "jpeg_roundtrip"
    _chk_image(who, x)
    N, Cc, H, W = x.shape
    if Cc != 3:
        raise ValueError(f"{who}: x must have 3 channels, got {Cc}")
    if H > 32768 or W > 32768 or N > 65535:
        raise ValueError(f"{who}: unsupported geometry N={N} H={H} W={W} (sides <= 32768, N <= 65535)")
    out = _chk_image_out(who, x, out, in_place=True)
    q = _per_image(who, "quality", quality, N, *JPEG_QUALITY_RANGE, "cpu")
    _chk_cuda(who, x, out)
    q = q.to(x.device)
    L.check(L.load().iir_jpeg_roundtrip_f32(x.data_ptr(), q.data_ptr(), N, Cc, H, W, out.data_ptr(), _stream()), "iir_jpeg_roundtrip_f32")
    return out


LPIPS_CPAD = L.MACROS["IIR_LPIPS_CPAD"]           # channels of the prepared image: the K tile the first conv reads
LPIPS_MAX_C = L.MACROS["IIR_LPIPS_MAX_C"]         # widest tap one wave holds
LPIPS_SHIFT = (-0.030, -0.088, -0.188)            # the scaling layer of LPIPS v0.1
LPIPS_SCALE = (0.458, 0.448, 0.450)


def _chk_rows16(who, name, t, rows, cols):
    """2-D fp16 / bf16 view of exactly `rows` rows and at least `cols` unit-stride columns whose rows a 16-byte access may address."""
    _refuse(who, torch.is_tensor(t) and t.dim() == 2 and t.dtype in _DT and t.stride(1) == 1 and t.shape[0] == rows and t.shape[1] >= cols
            and t.stride(0) % 8 == 0 and t.stride(0) >= cols,
            f"{name} must be a 2-D fp16 / bf16 view of {rows} rows and at least {cols} unit-stride columns with a row stride that is a "
            f"multiple of 8, got {getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))} {t.stride() if torch.is_tensor(t) else ()}")
    _refuse(who, not t.is_cuda or t.data_ptr() % 16 == 0, f"{name} must be 16-byte aligned")


def lpips_affine(device, shift=LPIPS_SHIFT, scale=LPIPS_SCALE):
    """The scaling layer as iir_lpips_prep reads it: fp64 (6,) = {shift[3], scale[3]} on `device`."""
    vals = [float(v) for v in tuple(shift) + tuple(scale)]
    if len(vals) != 6 or not all(v == v and abs(v) != float("inf") for v in vals) or any(v == 0.0 for v in vals[3:]):
        raise ValueError(f"lpips_affine: shift and scale must hold 3 finite values each, no scale 0, got {shift!r} {scale!r}")
    return torch.tensor(vals, dtype=torch.float64, device=device)


def lpips_prep(src, out, affine=None):
    """The scaling layer of LPIPS in front of VGG's first conv (iir_lpips_prep; DESIGN.md section 7 "LPIPS").  `src`: a contiguous
    source of `image_metrics` with 3 channels, fp32 (N, 3, H, W) in [0, 1] or uint8 (N, H, W, 3).  `out`: 2-D fp16 / bf16 view of
    N * H * W rows and at least LPIPS_CPAD columns: columns [0, 3) receive ((2 x - 1) - shift) / scale, [3, LPIPS_CPAD) zeros.
    `affine`: `lpips_affine(...)` (LPIPS's constants when absent)."""
    who = "lpips_prep"
    u8, (N, Cc, H, W) = _image_source(who, src, "src")
    _refuse(who, Cc == 3, f"src must have 3 channels, got {Cc}")
    _refuse(who, min(N, H, W) > 0 and max(H, W) <= 32768 and N * H * W * (LPIPS_CPAD // 8) <= 0x7fffffff * 256,
            f"unsupported geometry N={N} H={H} W={W}")
    _chk_rows16(who, "out", out, N * H * W, LPIPS_CPAD)
    if affine is not None:
        _refuse(who, torch.is_tensor(affine) and affine.dtype == torch.float64 and tuple(affine.shape) == (6,) and affine.is_contiguous(),
                "affine must be a contiguous fp64 (6,) tensor {shift[3], scale[3]} (lpips_affine)")
    _chk_cuda(who, src, out, *(() if affine is None else (affine,)))
    if affine is None:
        affine = lpips_affine(src.device)
    L.check(L.load().iir_lpips_prep(src.data_ptr(), int(u8), N, H, W, affine.data_ptr(), out.data_ptr(), out.stride(0), _DT[out.dtype],
                                    _stream()), "iir_lpips_prep")
    return out


def relu_(x):
    """In-place ReLU of a 2-D fp16 / bf16 view (iir_relu_f16): a negative value becomes +0, NaN stays; columns % 8 == 0."""
    who = "relu_"
    _refuse(who, torch.is_tensor(x) and x.dim() == 2 and min(x.shape) > 0, f"x must be a non-empty 2-D tensor, got {tuple(getattr(x, 'shape', ()))}")
    rows, Cc = x.shape
    _refuse(who, Cc % 8 == 0, f"the column count must be a multiple of 8, got {Cc}")
    _chk_rows16(who, "x", x, rows, Cc)
    _chk_cuda(who, x)
    L.check(L.load().iir_relu_f16(x.data_ptr(), x.stride(0), rows, Cc, _DT[x.dtype], _stream()), "iir_relu_f16")
    return x


def _chk_tap_geometry(who, pairs, H, W, Cc, count="pairs"):
    for name, v in ((count, pairs), ("H", H), ("W", W)):
        _refuse(who, not isinstance(v, bool) and isinstance(v, int) and v > 0, f"{name} must be a positive integer, got {v!r}")
    _refuse(who, pairs <= 65535 and max(H, W) <= 32768, f"unsupported geometry {count}={pairs} H={H} W={W} ({count} <= 65535, sides <= 32768)")
    _refuse(who, Cc > 0 and Cc % 8 == 0 and Cc <= LPIPS_MAX_C, f"the channel count must be a multiple of 8 up to {LPIPS_MAX_C}, got {Cc}")


def lpips_tap_workspace_bytes(pairs, H, W, C):
    """Bytes of fp64 partial sums `lpips_tap` needs for `pairs` image pairs of H x W pixels and C channels."""
    _chk_tap_geometry("lpips_tap_workspace_bytes", pairs, H, W, C)
    need = L.load().iir_lpips_tap_workspace_bytes(pairs, H, W, C)
    _refuse("lpips_tap_workspace_bytes", need >= 0, f"unsupported geometry pairs={pairs} H={H} W={W} C={C}")
    return int(need)


def lpips_tap(x, pairs, H, W, lin_w, pooled=None, dmap=None, ws=None, out=None):
    """One LPIPS tap (iir_lpips_tap; DESIGN.md section 7 "LPIPS").  `x`: 2-D fp16 / bf16 view of 2 * pairs * H * W rows, the
    pre-activation output of the tapped conv for the `a` images followed by their `b` partners; its column count C is the tap's
    width.  `lin_w`: fp32 (C,), the 1x1 `lin` layer.  Returns fp64 (pairs,): the mean over pixels of
    sum_c lin_w[c] (a^_c - b^_c)^2 on the unit-normalised ReLU outputs.  `dmap`: fp32 (pairs, H, W) that receives the per-pixel
    term; `pooled`: 2-D view of 2 * pairs * (H // 2) * (W // 2) rows and C columns that receives the 2x2 max-pooled ReLU output;
    `ws`: a byte workspace of at least `lpips_tap_workspace_bytes` (allocated here when absent)."""
    who = "lpips_tap"
    _refuse(who, torch.is_tensor(x) and x.dim() == 2, f"x must be a 2-D tensor, got {tuple(getattr(x, 'shape', ()))}")
    Cc = x.shape[1]
    _chk_tap_geometry(who, pairs, H, W, Cc)
    _chk_rows16(who, "x", x, 2 * pairs * H * W, Cc)
    _refuse(who, torch.is_tensor(lin_w) and lin_w.dtype == torch.float32 and tuple(lin_w.shape) == (Cc,) and lin_w.is_contiguous(),
            f"lin_w must be a contiguous fp32 ({Cc},) tensor, got {getattr(lin_w, 'dtype', type(lin_w))} {tuple(getattr(lin_w, 'shape', ()))}")
    tensors = [x, lin_w]
    if pooled is not None:
        _refuse(who, min(H, W) >= 2, f"a {H}x{W} tap has no 2x2 quad to pool")
        _chk_rows16(who, "pooled", pooled, 2 * pairs * (H // 2) * (W // 2), Cc)
        _refuse(who, pooled.dtype == x.dtype and pooled.shape[1] == Cc, f"pooled must have x's dtype and {Cc} columns")
        tensors.append(pooled)
    if dmap is not None:
        _refuse(who, torch.is_tensor(dmap) and dmap.dtype == torch.float32 and tuple(dmap.shape) == (pairs, H, W) and dmap.is_contiguous(),
                f"dmap must be a contiguous fp32 ({pairs}, {H}, {W}) tensor")
        tensors.append(dmap)
    if out is not None:
        _refuse(who, torch.is_tensor(out) and out.dtype == torch.float64 and tuple(out.shape) == (pairs,) and out.is_contiguous(),
                f"out must be a contiguous fp64 ({pairs},) tensor")
        tensors.append(out)
    _chk_cuda(who, *tensors)
    lo_x, hi_x = x.data_ptr(), x.data_ptr() + x.shape[0] * x.stride(0) * 2          # whole rows, as the entry counts them
    for name, t in (("pooled", pooled), ("dmap", dmap)):
        if t is not None:
            nbytes = t.shape[0] * t.stride(0) * 2 if t is pooled else t.numel() * 4
            _refuse(who, not (t.data_ptr() < hi_x and lo_x < t.data_ptr() + nbytes), f"{name} overlaps x (other pixels of x are still to be read)")
    h = L.load()
    need = h.iir_lpips_tap_workspace_bytes(pairs, H, W, Cc)
    _refuse(who, need >= 0, f"unsupported geometry pairs={pairs} H={H} W={W} C={Cc}")
    ws = _workspace(who, ws, need, x.device, where="x's device")
    if out is None:
        out = torch.empty(pairs, dtype=torch.float64, device=x.device)
    L.check(h.iir_lpips_tap(x.data_ptr(), x.stride(0), pairs, H, W, Cc, lin_w.data_ptr(), _DT[x.dtype], _p(dmap), _p(pooled),
                            0 if pooled is None else pooled.stride(0), ws.data_ptr(), ws.numel() * ws.element_size(), out.data_ptr(),
                            _stream()), "iir_lpips_tap")
    return out


DISTS_STATS = L.MACROS["IIR_DISTS_STATS"]         # sum a, sum b, sum a^2, sum b^2, sum ab
DISTS_MEAN = (0.485, 0.456, 0.406)                # the ImageNet normalisation in front of DISTS's trunk
DISTS_STD = (0.229, 0.224, 0.225)


def dists_affine(device, mean=DISTS_MEAN, std=DISTS_STD):
    """(x - mean) / std as `lpips_prep` computes it: ((2 x - 1) - shift) / scale with shift = 2 mean - 1, scale = 2 std."""
    return lpips_affine(device, tuple(2.0 * float(m) - 1.0 for m in mean), tuple(2.0 * float(s) for s in std))


def dists_l2pool(x, images, H, W, out=None):
    """DISTS's L2 pooling (iir_dists_l2pool; DESIGN.md section 7 "DISTS").  `x`: 2-D fp16 / bf16 view of images * H * W rows, the
    pre-activation output of a stage's last conv (the ReLU is applied on read); its column count C is the width.  Returns `out`, a
    2-D view of images * ceil(H / 2) * ceil(W / 2) rows and at least C columns of x's dtype (allocated here when absent):
    sqrt(hann3x3 * relu(x)^2 + 1e-12), stride 2, zero padding 1; columns past C keep their bits."""
    who = "dists_l2pool"
    _refuse(who, torch.is_tensor(x) and x.dim() == 2, f"x must be a 2-D tensor, got {tuple(getattr(x, 'shape', ()))}")
    Cc = x.shape[1]
    _chk_tap_geometry(who, images, H, W, Cc, count="images")
    _chk_rows16(who, "x", x, images * H * W, Cc)
    orows = images * ((H + 1) // 2) * ((W + 1) // 2)
    _refuse(who, orows * (Cc // 8) <= 0x7fffffff * 256, f"unsupported geometry images={images} H={H} W={W} C={Cc}")
    if out is None:
        out = torch.empty(orows, Cc, dtype=x.dtype, device=x.device)
    _chk_rows16(who, "out", out, orows, Cc)
    _refuse(who, out.dtype == x.dtype, f"out must have x's dtype {x.dtype}, got {out.dtype}")
    _chk_cuda(who, x, out)
    lo_x, hi_x = x.data_ptr(), x.data_ptr() + x.shape[0] * x.stride(0) * 2          # whole rows, as the entry counts them
    _refuse(who, not (out.data_ptr() < hi_x and lo_x < out.data_ptr() + orows * out.stride(0) * 2),
            "out overlaps x (other windows of x are still to be read)")
    L.check(L.load().iir_dists_l2pool(x.data_ptr(), x.stride(0), images, H, W, Cc, _DT[x.dtype], out.data_ptr(), out.stride(0), _stream()),
            "iir_dists_l2pool")
    return out


def dists_stats_workspace_bytes(pairs, H, W, C):
    """Bytes of fp64 partial sums `dists_stats` needs for `pairs` image pairs of H x W pixels and C channels."""
    _chk_tap_geometry("dists_stats_workspace_bytes", pairs, H, W, C)
    need = L.load().iir_dists_stats_workspace_bytes(pairs, H, W, C)
    _refuse("dists_stats_workspace_bytes", need >= 0, f"unsupported geometry pairs={pairs} H={H} W={W} C={C}")
    return int(need)


def _chk_stats_out(who, out, rows, Cc, tensors):
    if out is not None:
        _refuse(who, torch.is_tensor(out) and out.dtype == torch.float64 and tuple(out.shape) == (rows, Cc, DISTS_STATS) and out.is_contiguous(),
                f"out must be a contiguous fp64 ({rows}, {Cc}, {DISTS_STATS}) tensor")
        tensors.append(out)


def dists_stats(x, pairs, H, W, ws=None, out=None):
    """The per-channel sums DISTS compares (iir_dists_stats; DESIGN.md section 7 "DISTS").  `x`: 2-D fp16 / bf16 view of
    2 * pairs * H * W rows, the pre-activation output of a stage's last conv for the `a` images followed by their `b` partners
    (the ReLU is applied on read); its column count C is the width.  Returns fp64 (pairs, C, 5): {sum a, sum b, sum a^2, sum b^2,
    sum ab} over the H * W pixels, every product and sum in fp64.  `ws`: a byte workspace of at least
    `dists_stats_workspace_bytes` (allocated here when absent)."""
    who = "dists_stats"
    _refuse(who, torch.is_tensor(x) and x.dim() == 2, f"x must be a 2-D tensor, got {tuple(getattr(x, 'shape', ()))}")
    Cc = x.shape[1]
    _chk_tap_geometry(who, pairs, H, W, Cc)
    _chk_rows16(who, "x", x, 2 * pairs * H * W, Cc)
    tensors = [x]
    _chk_stats_out(who, out, pairs, Cc, tensors)
    _chk_cuda(who, *tensors)
    h = L.load()
    need = h.iir_dists_stats_workspace_bytes(pairs, H, W, Cc)
    _refuse(who, need >= 0, f"unsupported geometry pairs={pairs} H={H} W={W} C={Cc}")
    ws = _workspace(who, ws, need, x.device, where="x's device")
    if out is None:
        out = torch.empty(pairs, Cc, DISTS_STATS, dtype=torch.float64, device=x.device)
    L.check(h.iir_dists_stats(x.data_ptr(), x.stride(0), pairs, H, W, Cc, _DT[x.dtype], ws.data_ptr(), ws.numel() * ws.element_size(),
                              out.data_ptr(), _stream()), "iir_dists_stats")
    return out


def _chk_image_pair(who, a, b):
    u8, da = _image_source(who, a, "a")
    u8b, db = _image_source(who, b, "b")
    _refuse(who, u8 == u8b and da == db, f"a and b must share a dtype and a shape, got {a.dtype} {tuple(a.shape)} and {b.dtype} {tuple(b.shape)}")
    N, Cc, H, W = da
    _refuse(who, Cc == 3, f"a and b must have 3 channels, got {Cc}")
    _refuse(who, min(N, H, W) > 0 and N <= 65535 and max(H, W) <= 32768, f"unsupported geometry N={N} H={H} W={W} (N <= 65535, sides <= 32768)")
    return u8, N, H, W


def dists_image_stats_workspace_bytes(N, H, W):
    """Bytes of fp64 partial sums `dists_image_stats` needs for N image pairs of H x W pixels."""
    _chk_tap_geometry("dists_image_stats_workspace_bytes", N, H, W, 8, count="N")
    need = L.load().iir_dists_image_stats_workspace_bytes(N, H, W)
    _refuse("dists_image_stats_workspace_bytes", need >= 0, f"unsupported geometry N={N} H={H} W={W}")
    return int(need)


def dists_image_stats(a, b, ws=None, out=None):
    """`dists_stats` of DISTS's stage 0, the raw images (iir_dists_image_stats): `a`, `b` contiguous sources of `image_metrics`
    with 3 channels, both fp32 (N, 3, H, W) in [0, 1] or both uint8 (N, H, W, 3) (x = u / 255 in fp32: a uint8 image and its fp32
    copy give equal bits).  Returns fp64 (N, 3, 5)."""
    who = "dists_image_stats"
    u8, N, H, W = _chk_image_pair(who, a, b)
    tensors = [a, b]
    _chk_stats_out(who, out, N, 3, tensors)
    _chk_cuda(who, *tensors)
    h = L.load()
    need = h.iir_dists_image_stats_workspace_bytes(N, H, W)
    _refuse(who, need >= 0, f"unsupported geometry N={N} H={H} W={W}")
    ws = _workspace(who, ws, need, a.device, where="the images' device")
    if out is None:
        out = torch.empty(N, 3, DISTS_STATS, dtype=torch.float64, device=a.device)
    L.check(h.iir_dists_image_stats(a.data_ptr(), b.data_ptr(), int(u8), N, H, W, ws.data_ptr(), ws.numel() * ws.element_size(), out.data_ptr(),
                                    _stream()), "iir_dists_image_stats")
    return out
