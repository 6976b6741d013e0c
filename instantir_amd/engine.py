"""MI355X executors for the two networks of the InstantIR step: SDXL UNet with TA-IP decoupled
cross-attention (`HipUNet`) and the Aggregator (`HipAggregator`).

Python here only sequences C-ABI kernel launches (instantir_amd.ops) over pre-packed fp16 weights
and a bump-allocated activation arena; every launch goes to torch's current stream, so a whole
denoising step can be captured into a hipGraph by the caller.  There is no torch arithmetic on
the forward path.

Reference behaviour reproduced (citations to /root/reference):
  * UNet forward: module/unet/unet_2d_ZeroSFT.py:1226-1388 structure with stock-diffusers additive
    ControlNet residuals; leaf math module/min_sdxl.py:242-283 (resnet),
    :531-595 (transformer), :598-618 (down/upsample).
  * attention processors: module/ip_adapter/attention_processor.py:337-414, :1093-1207, :6-26.
  * Aggregator: module/aggregator.py:758-977 (+ SFT :70-90, zero 1x1 :414-417), attn2 removed
    (pipelines/sdxl_instantir.py:165-177).
  * Resampler: module/ip_adapter/resampler.py:34-78,127-147 via MultiIPAdapterImageProjection
    (module/ip_adapter/ip_adapter.py:68-90).

MI355X-first restructuring (observable results unchanged):
  * NHWC activations: a feature map IS its token matrix; no permutes around Transformer2D.
  * step-invariant work hoisted out of the step: Resampler, text K/V
    projections, to_k_ip/to_v_ip projections, add_embedding branch.
  * all resnet time_emb_proj linears and all adaLN linears of a network are each ONE GEMM per forward.
  * q|k projections fused into one GEMM; V is produced transposed (V^T = Wv . X^T) for the
    attention kernel; GEGLU, SiLU, bias, temb add and residual adds live in GEMM/conv epilogues;
    skip concatenation is written in place by the producer and the ControlNet residual add is
    folded into the skip copy.
"""
from __future__ import annotations

import os

from typing import Dict, List, Optional

import torch

from . import ops, pag, seg
from .config import UNetConfig
from .packing import conv_weight_nhwc, pair_rows
from .weights import skip_channels

F16 = torch.float16
CPAD = 64          # latent channels are zero-padded to one K tile


class _NullOps:
    """Stand-in for `ops` during the arena-sizing dry run: every launch is skipped."""

    def __getattr__(self, name):
        return lambda *a, **k: None


class Arena:
    """Bump allocator over one fp16 device buffer.  Static op order => static addresses, which is
    what hipGraph capture needs."""

    def __init__(self, device, dtype=F16):
        self.device = device
        self.dtype = dtype
        self.buf = None
        self.off = 0
        self.high = 0

    def reserve(self, n_elems):
        self.buf = torch.empty(n_elems, dtype=self.dtype, device=self.device)

    def alloc(self, rows, cols):
        n = (rows * cols + 127) // 128 * 128
        off = self.off
        self.off += n
        self.high = max(self.high, self.off)
        if self.buf is None:      # dry run: hand out a meta view so shapes/strides still work
            return torch.empty(rows, cols, dtype=self.dtype, device="meta")
        if self.off > self.buf.numel():
            raise RuntimeError("activation arena overflow (forward differs from its sizing run)")
        return self.buf[off:off + rows * cols].view(rows, cols)

    def mark(self):
        return self.off

    def release(self, m):
        self.off = m

    def reset(self):
        self.off = 0


def _merge_lora(sd: Dict[str, torch.Tensor], lora: Dict[str, torch.Tensor], scaling: float) -> Dict[str, torch.Tensor]:
    """W' = W + s * B A (linear) / W'[o,i,:,:] = W + s * sum_r B[o,r] A[r,i,:,:] (conv): the enabled-adapter
    forward of peft folded into a second weight copy.  The rank-r product runs on this
    library's own GEMM (`iir_gemm_f16`: fp32 accumulation, W added as the epilogue's residual) -- no vendor BLAS on the
    product's set-up path either.  The rank is zero-padded to one K tile (64)."""
    out = dict(sd)
    for k in lora:
        if not k.endswith(".lora_A.weight"):
            continue
        path = k[: -len(".lora_A.weight")]
        w = sd[path + ".weight"]
        dev = w.device
        if not w.is_cuda:
            raise RuntimeError("_merge_lora: weights must be on the GPU (the merge runs in the HIP library)")
        a, b = lora[k].to(dev), lora[path + ".lora_B.weight"].to(dev)
        r = a.shape[0]
        rp = (r + 63) // 64 * 64
        n_out = w.shape[0]
        kk = w.numel() // n_out
        bs = torch.zeros(n_out, rp, dtype=F16, device=dev)                      # s * B, [N][r]
        bs[:, :r] = (b.reshape(n_out, r).float() * scaling).to(F16)
        at = torch.zeros(kk, rp, dtype=F16, device=dev)                         # A^T, [K][r]: the GEMM's "weight" operand
        at[:, :r] = a.reshape(r, kk).t().to(F16)
        w2 = w.reshape(n_out, kk).to(F16).contiguous()
        merged = torch.empty_like(w2)
        ops.gemm(bs, at, merged, res=w2)
        out[path + ".weight"] = merged.reshape(w.shape).to(w.dtype)
    return out


class _RecDict(dict):
    """Weight dict that reports every lookup (used once, in the dry run, to learn the order of use)."""

    def __init__(self, base, note):
        super().__init__(base)
        self._note = note

    def __getitem__(self, k):
        self._note(k)
        return dict.__getitem__(self, k)


class _Net:
    """Shared machinery: packed weights, arena, resnet / transformer executors."""

    def __init__(self, cfg: UNetConfig, sd: Dict[str, torch.Tensor], cross: bool, device, fp8_linear: bool = False):
        self.cfg = cfg
        self.cross = cross
        self.device = device
        self.fp8_linear = fp8_linear      # BASELINE configs[4]: transformer linears as fp8-E4M3 weights (iir_gemm_desc.wscale)
        self.arena = Arena(device)
        self.o = ops
        self.w: Dict[str, torch.Tensor] = {}
        self._temb_slices: Dict[str, slice] = {}
        self._ada_slices: Dict[str, slice] = {}
        # weight streaming state: `units` = (ptr, bytes) of the weights first used by each resnet /
        # transformer block / SFT head, in execution order inside ONE contiguous weight arena
        self.units: List[tuple] = []
        self._use_log: Optional[list] = None
        self._gnws = None
        self._warena = None
        self.arena_gen = 0
        # LayerNorm folded into the GEMMs either side of it (ops.LnFold; iir_gemm_desc.ln_stats_out / ln_stats_in): not with fp8
        # operands (the activation would be rounded to 3 mantissa bits BEFORE its row mean is removed)
        self.ln_fold = not fp8_linear
        # perturbed-attention guidance: None, or (frozenset of selected `attn1` paths, ident_from) -- set on the main UNet only
        # (HipUNet.set_pag)
        self.pag = None
        # smoothed-energy guidance: None, or a `_SegState` -- the other way to perturb those rows (HipUNet.set_seg); never both
        self.seg = None
        # The two launch-path options a caller may set (both are part of the pipeline's loop key).  `inkernel_prefetch`: GEMMs and
        # convs pull the weights that follow their own towards the Infinity Cache (`_pf`).
        # `fp8_act`, fp8 build (BASELINE configs[4]): the activations of the transformer linears are STORED as fp8 by the launch that
        # produces them (LayerNorm, attention, GEGLU) and both operands enter the MFMA as fp8 (`ops.gemm_fp8`): the same operand bytes
        # the fp8-weight GEMM formed in registers from fp16 activations (identical results), half the 128-byte lines per FLOP.
        # IIR_FP8_ACT=0 builds the register-conversion form (the reference side of the full-size fp8 test).
        self.inkernel_prefetch = True
        self.fp8_act = fp8_linear and os.environ.get("IIR_FP8_ACT", "1") != "0"
        self._pack_encoder(sd)

    # ---- weight packing ---------------------------------------------------------------------
    def _t(self, sd, name):
        return sd[name].to(device=self.device, dtype=F16)

    def _qw(self, sd, name):
        """q-projection weight x (head_dim^-1/2 * log2 e), formed in fp32, stored fp16."""
        f = ops.attn_q_factor(self.cfg.head_dim ** -0.5)
        return (sd[name].to(device=self.device, dtype=torch.float32) * f).to(F16)

    def _pack_linear(self, sd, path, dst=None):
        dst = dst or path
        self.w[dst + ".w"] = self._t(sd, path + ".weight").contiguous()
        if (path + ".bias") in sd:
            self.w[dst + ".b"] = self._t(sd, path + ".bias").contiguous()

    def _pack_conv3(self, sd, path, cin_pad=None):
        self.w[path + ".w"] = conv_weight_nhwc(self._t(sd, path + ".weight"), cin_pad)
        self.w[path + ".b"] = self._t(sd, path + ".bias").contiguous()

    def _pack_fold(self, dst, w32, sd, norm, bias=None, pair=None):
        """`dst`.lnw / .lnb / .lncs: the Linear `w32` with the LayerNorm `norm` folded in (ops.LnFold)."""
        f = ops.LnFold(w32, sd[norm + ".weight"].to(self.device), sd[norm + ".bias"].to(self.device), bias=bias, eps=1e-5, pair=pair)
        self.w[dst + ".lnw"], self.w[dst + ".lnb"], self.w[dst + ".lncs"] = f.w, f.bias, f.colsum

    def _pack_norm(self, sd, path):
        self.w[path + ".g"] = self._t(sd, path + ".weight").contiguous()
        self.w[path + ".b"] = self._t(sd, path + ".bias").contiguous()

    def _pack_resnet(self, sd, path, temb_list):
        self._pack_norm(sd, path + ".norm1")
        self._pack_conv3(sd, path + ".conv1")
        self._pack_norm(sd, path + ".norm2")
        self._pack_conv3(sd, path + ".conv2")
        temb_list.append((path, self._t(sd, path + ".time_emb_proj.weight"), self._t(sd, path + ".time_emb_proj.bias")))
        if (path + ".conv_shortcut.weight") in sd:
            w = self._t(sd, path + ".conv_shortcut.weight")
            self.w[path + ".conv_shortcut.w"] = w.reshape(w.shape[0], w.shape[1]).contiguous()
            self.w[path + ".conv_shortcut.b"] = self._t(sd, path + ".conv_shortcut.bias").contiguous()

    def _pack_transformer(self, sd, path, depth, ada_list):
        self._pack_norm(sd, path + ".norm")
        self._pack_linear(sd, path + ".proj_in")
        self._pack_linear(sd, path + ".proj_out")
        for k in range(depth):
            p = f"{path}.transformer_blocks.{k}"
            self._pack_norm(sd, p + ".norm1")
            # one projection for q | k | v: the V third is written transposed by the GEMM's epilogue (iir_gemm_desc.Ct)
            # (the softmax scale x log2 e is folded into the q rows: the attention kernel takes Q as it stands, `q_prescaled`)
            self.w[p + ".attn1.qkv.w"] = torch.cat([self._qw(sd, p + ".attn1.to_q.weight"), self._t(sd, p + ".attn1.to_k.weight"),
                                                    self._t(sd, p + ".attn1.to_v.weight")], 0).contiguous()
            f32 = lambda n_: sd[n_].to(device=self.device, dtype=torch.float32)
            qf = ops.attn_q_factor(self.cfg.head_dim ** -0.5)
            if self.ln_fold:       # norm1 -> q|k|v, norm2 -> to_q, norm3 -> GEGLU proj: gamma into the weight, beta into a bias (fp32, one rounding)
                self._pack_fold(p + ".attn1.qkv", torch.cat([f32(p + ".attn1.to_q.weight") * qf, f32(p + ".attn1.to_k.weight"),
                                                             f32(p + ".attn1.to_v.weight")], 0), sd, p + ".norm1")
            self._pack_linear(sd, p + ".attn1.to_out.0")
            if self.cross:
                self._pack_norm(sd, p + ".norm2")
                if self.ln_fold:
                    self._pack_fold(p + ".attn2.to_q", f32(p + ".attn2.to_q.weight") * qf, sd, p + ".norm2")
                self.w[p + ".attn2.to_q.w"] = self._qw(sd, p + ".attn2.to_q.weight").contiguous()
                self._pack_linear(sd, p + ".attn2.to_k")
                self._pack_linear(sd, p + ".attn2.to_v")
                self._pack_linear(sd, p + ".attn2.to_out.0")
                pp = p + ".attn2.processor"
                self._pack_linear(sd, pp + ".to_k_ip")
                self._pack_linear(sd, pp + ".to_v_ip")
                for kv in ("k", "v"):
                    ada_list.append((f"{p}.{kv}", self._t(sd, f"{pp}.ln_{kv}_ip.linear.weight"), self._t(sd, f"{pp}.ln_{kv}_ip.linear.bias")))
            self._pack_norm(sd, p + ".norm3")
            w1, b1 = self._t(sd, p + ".ff.net.0.proj.weight"), self._t(sd, p + ".ff.net.0.proj.bias")
            n = w1.shape[0] // 2
            self.w[p + ".ff1.w"] = pair_rows(w1[:n], w1[n:])          # GEGLU: value rows | gate rows
            self.w[p + ".ff1.b"] = pair_rows(b1[:n], b1[n:])
            if self.ln_fold:
                self._pack_fold(p + ".ff1", f32(p + ".ff.net.0.proj.weight"), sd, p + ".norm3", bias=f32(p + ".ff.net.0.proj.bias"), pair=pair_rows)
            self._pack_linear(sd, p + ".ff.net.2", p + ".ff2")
            if self.fp8_linear:
                for key in ([p + ".attn1.qkv.w", p + ".attn1.to_out.0.w", p + ".ff1.w", p + ".ff2.w"]
                            + ([p + ".attn2.to_q.w", p + ".attn2.to_out.0.w"] if self.cross else [])):
                    self.w[key] = ops.Fp8Weight(*ops.quantize_fp8_rows(self.w[key]))
        if self.fp8_linear:
            for key in (path + ".proj_in.w", path + ".proj_out.w"):
                self.w[key] = ops.Fp8Weight(*ops.quantize_fp8_rows(self.w[key]))

    def _pack_encoder(self, sd):
        cfg = self.cfg
        self._temb, self._ada = [], []
        self._pack_conv3(sd, "conv_in", CPAD)
        for n in ("time_embedding.linear_1", "time_embedding.linear_2", "add_embedding.linear_1", "add_embedding.linear_2"):
            self._pack_linear(sd, n)
        nb = len(cfg.block_out_channels)
        for i in range(nb):
            for j in range(cfg.layers_per_block):
                self._pack_resnet(sd, f"down_blocks.{i}.resnets.{j}", self._temb)
                if cfg.transformer_depth[i] > 0:
                    self._pack_transformer(sd, f"down_blocks.{i}.attentions.{j}", cfg.transformer_depth[i], self._ada)
            if i < nb - 1:
                self._pack_conv3(sd, f"down_blocks.{i}.downsamplers.0.conv")
        self._pack_resnet(sd, "mid_block.resnets.0", self._temb)
        self._pack_transformer(sd, "mid_block.attentions.0", cfg.mid_depth, self._ada)
        self._pack_resnet(sd, "mid_block.resnets.1", self._temb)

    def _finish_pack(self):
        """Concatenate every time_emb_proj (and every adaLN linear) into one weight: one GEMM per forward."""
        off, ws, bs = 0, [], []
        for path, w, b in self._temb:
            self._temb_slices[path] = slice(off, off + w.shape[0])
            off += w.shape[0]
            ws.append(w); bs.append(b)
        self.w["temb_all.w"] = torch.cat(ws, 0).contiguous()
        self.w["temb_all.b"] = torch.cat(bs, 0).contiguous()
        if self._ada:
            off, ws, bs = 0, [], []
            for key, w, b in self._ada:
                self._ada_slices[key] = slice(off, off + w.shape[0])
                off += w.shape[0]
                ws.append(w); bs.append(b)
            self.w["ada_all.w"] = torch.cat(ws, 0).contiguous()
            self.w["ada_all.b"] = torch.cat(bs, 0).contiguous()
        del self._temb, self._ada

    # ---- arena sizing -----------------------------------------------------------------------
    def _size_arena(self, fn):
        """Dry-run `fn` (launches skipped) to find the arena high-water mark, then allocate it."""
        self.arena.buf, self.arena.off, self.arena.high = None, 0, 0
        self.arena_gen = getattr(self, "arena_gen", 0) + 1        # launch sequences captured on the previous arena are stale
        self.o = _NullOps()
        plain = self.w
        first = not self.units
        self._gnws = ops.gn_workspace(self.device, 64, self.cfg.norm_groups)
        if first:
            self._use_log = []
            self.w = _RecDict(plain, lambda k: self._use_log.append(k))
        try:
            fn()
        finally:
            self.o = ops
            self.w = plain
        if first:
            self._consolidate_weights()
        self.arena.reserve(self.arena.high + 1024)
        self.arena.reset()

    def _consolidate_weights(self):
        """Re-home every packed weight into one contiguous fp16 arena ordered by first use in the forward
        (so the weights of a block are one address range the prefetcher can pull ahead of the GEMMs)."""
        order, seen, marks = [], set(), []
        for k in self._use_log:
            if isinstance(k, tuple):            # ("unit", name) marker
                marks.append(len(order))
            elif k not in seen:
                seen.add(k)
                order.append(k)
        order += [k for k in self.w if k not in seen]
        order = [k for k in order if torch.is_tensor(self.w[k]) and self.w[k].dtype == F16]      # (fp8 weights stay where they are)
        al = lambda n: (n + 127) // 128 * 128
        offs, tot = [], 0
        for k in order:
            offs.append(tot)
            tot += al(self.w[k].numel())
        arena = torch.empty(tot, dtype=F16, device=self.device)
        for k, off in zip(order, offs):
            t = self.w[k]
            v = arena[off:off + t.numel()].view(t.shape)
            v.copy_(t)
            self.w[k] = v
        self._warena = arena
        self.units = [None]                 # (consolidated: `_size_arena` records the order of use only once)
        self._use_log = None

    def _unit(self, name):
        """Called at the start of every resnet / transformer block / SFT head: marks where a block's weights begin in the
        execution-ordered weight arena (recorded once, in the sizing dry run).  (A side-stream prefetcher used to hang off
        these marks; it measured slower under graph replay and its third-stream fork inside a capture crashed
        hipStreamEndCapture, so it was removed in round 2 -- the in-kernel tail prefetch `_pf` is the form that pays.)"""
        if self._use_log is not None:
            self._use_log.append(("unit", name))

    def _pf(self, wt):
        """(ptr, bytes) of the weight-arena range a launch using `wt` should pull towards the Infinity Cache:
        as many bytes as it consumes itself, starting right after its own weights in the (execution-ordered) arena."""
        if not self.inkernel_prefetch or self._warena is None or self.o is not ops:
            return None
        base, end = self._warena.data_ptr(), self._warena.data_ptr() + self._warena.numel() * 2
        n = wt.numel() * 2
        lo = wt.data_ptr() + n
        if lo < base or lo >= end or n < (256 << 10):
            return None
        return (lo, min(n, end - lo))

    def _begin(self):
        self.arena.reset()

    def _gn_tag(self, y, hw, K, conv):
        """GroupNorm statistics from the launch that produces the GroupNorm's input (ops.gemm / conv2d `gn_out=`): arena room for
        the partials of `y` (rows, C), about to be written by a (rows, C, K) launch -- fp32 (rows / 64, C, 2) -- tagged onto `y`
        so that the GroupNorm which consumes it skips its statistics pass (`_gn_of`), and returned for the producer's `gn_out=`.
        None, and the three-launch GroupNorm, when the fused path does not apply (images not made of whole 64-row slabs, tiles that
        cannot emit the partials).  Allocation happens in the sizing dry run as well: static addresses."""
        rows, C = y.shape
        if hw % 64 or self.arena.dtype != F16 or not ops.gn_supported(rows, C, K, conv):
            return None
        if (hw // 64) * (C // self.cfg.norm_groups) > ops.GN_PARTIALS_MAX:         # iir_groupnorm_from_partials merges at most this many per (image, group)
            return None
        y._gn_parts = self.arena.alloc(rows // 64 * C, 4).view(torch.float32).view(rows // 64, C, 2)
        return y._gn_parts

    @staticmethod
    def _gn_of(x):
        return getattr(x, "_gn_parts", None)

    # ---- blocks -----------------------------------------------------------------------------
    def _resnet(self, path, x, R, H, W, temb_all, out=None, eps=1e-5):
        """x (R*H*W, Cin) view -> (R*H*W, Cout).  module/min_sdxl.py:261-283."""
        self._unit(path)
        o, w, A = self.o, self.w, self.arena
        HW = H * W
        cin = x.shape[1]
        cout = w[path + ".conv1.w"].shape[0]
        if out is None:
            out = A.alloc(R * HW, cout)
        p_out = self._gn_tag(out, HW, 9 * cout, True)            # partials of this block's output
        m = A.mark()
        h = A.alloc(R * HW, cin)
        o.groupnorm(x, h, R, HW, w[path + ".norm1.g"], w[path + ".norm1.b"], eps, True, self.cfg.norm_groups, self._gnws,
                    partials=self._gn_of(x))
        h2 = A.alloc(R * HW, cout)
        o.conv2d(h.view(R, H, W, cin), w[path + ".conv1.w"], h2, bias=w[path + ".conv1.b"],
                 rowbias=temb_all[:, self._temb_slices[path]], rows_per_rb=HW, prefetch=self._pf(w[path + ".conv1.w"]),
                 gn_out=self._gn_tag(h2, HW, 9 * cin, True))
        h3 = A.alloc(R * HW, cout)
        o.groupnorm(h2, h3, R, HW, w[path + ".norm2.g"], w[path + ".norm2.b"], eps, True, self.cfg.norm_groups, self._gnws,
                    partials=self._gn_of(h2))
        if (path + ".conv_shortcut.w") in w:
            sc = A.alloc(R * HW, cout)
            o.gemm(x, w[path + ".conv_shortcut.w"], sc, bias=w[path + ".conv_shortcut.b"])
        else:
            sc = x
        o.conv2d(h3.view(R, H, W, cout), w[path + ".conv2.w"], out, bias=w[path + ".conv2.b"], res=sc,
                 prefetch=self._pf(w[path + ".conv2.w"]), gn_out=p_out)
        A.release(m)
        return out

    def _tblock(self, p, h, R, T, heads, st, ada, lnst=None, last=False, grid=None):
        """One BasicTransformerBlock in place on h (R*T, C).  module/min_sdxl.py:541-562.  `grid`: (H, W) of the token grid.
        `lnst` (fp32 (parts, M, 2)): the LayerNorm partials of `h` left by the GEMM that wrote it.  When given, no LayerNorm
        kernel runs in this block: each of the three norms is folded into the GEMM behind it (reads raw `h`, `ln_in`) and each
        GEMM that writes `h` refreshes the partials (`ln_out`) for the next norm -- also the next block's, unless `last`."""
        self._unit(p)
        o, w, A = self.o, self.w, self.arena
        C = h.shape[1]
        M = R * T
        m = A.mark()
        fold = lnst is not None
        if self.fp8_act and not fold and C % 128 == 0 and isinstance(w[p + ".attn1.qkv.w"], ops.Fp8Weight) and h.dtype == F16:
            assert self.pag is None and self.seg is None           # (set_pag / set_seg refuse fp8 engines)
            self._tblock_fp8(p, h, R, T, heads, st)
            A.release(m)
            return
        n = None if fold else A.alloc(M, C)
        # -- self-attention (AttnProcessor2_0, attention_processor.py:370-402)
        qk = A.alloc(M, 2 * C)
        vt = A.alloc(C, M)
        if fold:
            wqkv = w[p + ".attn1.qkv.lnw"]
            o.gemm(h, wqkv, qk, bias=w[p + ".attn1.qkv.lnb"], prefetch=self._pf(wqkv), out_t=(vt, 2 * C),
                   ln_in=(lnst, w[p + ".attn1.qkv.lncs"], 1e-5))
        else:
            o.layernorm(h, n, w[p + ".norm1.g"], w[p + ".norm1.b"], 1e-5)
            wqkv = w[p + ".attn1.qkv.w"]
            o.gemm(n, wqkv, qk, prefetch=self._pf(wqkv), out_t=(vt, 2 * C))                 # q | k, and V^T from the same launch
        a = A.alloc(M, C)
        # PAG: the perturbed rows [ident_from, R) of a selected attn1 get the identity attention map, a = v, in the same launch
        ident = self.pag[1] if self.pag is not None and (p + ".attn1") in self.pag[0] else 0
        # SEG: the queries of the perturbed rows [first, R) of a selected attn1 are blurred over the token grid, in place in the
        # q columns the projection just wrote; the attention launch then is the plain one for every row
        sg = self.seg
        if sg is not None and (p + ".attn1") in sg.paths:
            wy, wx = (None, None) if sg.mean else (sg.taps[grid[0]], sg.taps[grid[1]])
            o.seg_blur_q(qk[sg.first * T:, :C], R - sg.first, grid[0], grid[1], wy, wx, mean=sg.mean)
        o.attention(qk[:, :C], a, [(qk[:, C:], T, vt, T, T)], R, heads, T, q_prescaled=True, ident_from=ident)
        o.gemm(a, w[p + ".attn1.to_out.0.w"], h, bias=w[p + ".attn1.to_out.0.b"], res=h,
               prefetch=self._pf(w[p + ".attn1.to_out.0.w"]), ln_out=lnst)
        # -- decoupled cross-attention (TA_IPAttnProcessor2_0, attention_processor.py:1140-1195)
        if self.cross:
            q = qk[:, :C]
            cfg = self.cfg
            nip, ipad = cfg.num_ip_tokens, (cfg.num_ip_tokens + 7) // 8 * 8
            kv = st["kv"][p]
            ipk, ipvt = kv["ipk"], kv["ipvt"]          # adaLN'd for this step by the batched launch in _embeddings
            segs = [(kv["tk"], cfg.text_len, kv["tvt"], kv["tpad"], cfg.text_len), (ipk, nip, ipvt, ipad, nip)]
            wq = w[p + (".attn2.to_q.lnw" if fold else ".attn2.to_q.w")]
            # to_q and the text / IP cross-attention in ONE launch (IIR_EPI_XATTN): every workgroup finishes a 64-row x 2-head
            # tile of q and attends with it; q never goes to memory and 174 launches per step disappear
            fuse = (cfg.head_dim == 64 and C % 128 == 0 and T % 64 == 0 and cfg.text_len <= 80 and nip <= 64 and h.dtype == F16
                    and not isinstance(wq, ops.Fp8Weight))
            if not fold:
                o.layernorm(h, n, w[p + ".norm2.g"], w[p + ".norm2.b"], 1e-5)
            src = h if fold else n
            kw = dict(bias=w[p + ".attn2.to_q.lnb"], ln_in=(lnst, w[p + ".attn2.to_q.lncs"], 1e-5)) if fold else {}
            if fuse:
                o.gemm(src, wq, a, prefetch=self._pf(wq), epi=ops.EPI_XATTN, xattn=(segs, T), **kw)
            else:
                o.gemm(src, wq, q, prefetch=self._pf(wq), **kw)
                o.attention(q, a, segs, R, heads, T, q_prescaled=True)
            o.gemm(a, w[p + ".attn2.to_out.0.w"], h, bias=w[p + ".attn2.to_out.0.b"], res=h,
                   prefetch=self._pf(w[p + ".attn2.to_out.0.w"]), ln_out=lnst)
        # -- GEGLU feed-forward (module/min_sdxl.py:502-528)
        f = A.alloc(M, 4 * C)
        if fold:
            o.gemm(h, w[p + ".ff1.lnw"], f, bias=w[p + ".ff1.lnb"], epi=ops.EPI_GEGLU, prefetch=self._pf(w[p + ".ff1.lnw"]),
                   ln_in=(lnst, w[p + ".ff1.lncs"], 1e-5))
        else:
            o.layernorm(h, n, w[p + ".norm3.g"], w[p + ".norm3.b"], 1e-5)
            o.gemm(n, w[p + ".ff1.w"], f, bias=w[p + ".ff1.b"], epi=ops.EPI_GEGLU, prefetch=self._pf(w[p + ".ff1.w"]))
        o.gemm(f, w[p + ".ff2.w"], h, bias=w[p + ".ff2.b"], res=h, prefetch=self._pf(w[p + ".ff2.w"]), ln_out=None if last else lnst)
        A.release(m)

    def _tblock_fp8(self, p, h, R, T, heads, st):
        """The block of `_tblock` with fp8 operands on both sides of its six linears (module/min_sdxl.py:541-562; fp8 build only):
        LayerNorm / attention / GEGLU store their outputs as E4M3 bytes, `ops.gemm_fp8` consumes them."""
        o, w, A, cfg = self.o, self.w, self.arena, self.cfg
        C, M = h.shape[1], R * T
        a8 = lambda rows, cols: A.alloc(rows, cols // 2).view(torch.uint8).view(rows, cols)      # byte matrix in the fp16 arena
        n8 = a8(M, C)
        qk = A.alloc(M, 2 * C)
        vt = A.alloc(C, M)
        o.layernorm(h, n8, w[p + ".norm1.g"], w[p + ".norm1.b"], 1e-5)
        wqkv = w[p + ".attn1.qkv.w"]
        o.gemm_fp8(n8, wqkv, qk, prefetch=self._pf(wqkv), out_t=(vt, 2 * C))
        at8 = a8(M, C)
        o.attention(qk[:, :C], at8, [(qk[:, C:], T, vt, T, T)], R, heads, T, q_prescaled=True)
        o.gemm_fp8(at8, w[p + ".attn1.to_out.0.w"], h, bias=w[p + ".attn1.to_out.0.b"], res=h, prefetch=self._pf(w[p + ".attn1.to_out.0.w"]))
        if self.cross:
            q = qk[:, :C]
            nip, ipad = cfg.num_ip_tokens, (cfg.num_ip_tokens + 7) // 8 * 8
            kv = st["kv"][p]
            o.layernorm(h, n8, w[p + ".norm2.g"], w[p + ".norm2.b"], 1e-5)
            o.gemm_fp8(n8, w[p + ".attn2.to_q.w"], q, prefetch=self._pf(w[p + ".attn2.to_q.w"]))
            o.attention(q, at8, [(kv["tk"], cfg.text_len, kv["tvt"], kv["tpad"], cfg.text_len), (kv["ipk"], nip, kv["ipvt"], ipad, nip)],
                        R, heads, T, q_prescaled=True)
            o.gemm_fp8(at8, w[p + ".attn2.to_out.0.w"], h, bias=w[p + ".attn2.to_out.0.b"], res=h, prefetch=self._pf(w[p + ".attn2.to_out.0.w"]))
        o.layernorm(h, n8, w[p + ".norm3.g"], w[p + ".norm3.b"], 1e-5)
        if ops.fp8_out_supported(M, 8 * C, C, True):
            f8 = a8(M, 4 * C)
            o.gemm_fp8(n8, w[p + ".ff1.w"], f8, bias=w[p + ".ff1.b"], epi=ops.EPI_GEGLU, prefetch=self._pf(w[p + ".ff1.w"]))
            o.gemm_fp8(f8, w[p + ".ff2.w"], h, bias=w[p + ".ff2.b"], res=h, prefetch=self._pf(w[p + ".ff2.w"]))
        else:             # ragged tiles (small test geometries): fp16 GEGLU output, converted by the fp8-weight GEMM in registers
            f = A.alloc(M, 4 * C)
            o.gemm_fp8(n8, w[p + ".ff1.w"], f, bias=w[p + ".ff1.b"], epi=ops.EPI_GEGLU, prefetch=self._pf(w[p + ".ff1.w"]))
            o.gemm(f, w[p + ".ff2.w"], h, bias=w[p + ".ff2.b"], res=h, prefetch=self._pf(w[p + ".ff2.w"]))

    def _transformer(self, path, x, depth, R, H, W, st, ada, out=None):
        """Transformer2DModel on the NHWC map x (R*H*W, C).  module/min_sdxl.py:578-595."""
        o, w, A = self.o, self.w, self.arena
        C = x.shape[1]
        T = H * W
        if out is None:
            out = A.alloc(R * T, C)
        # partials of the block's output (proj_out + residual); an fp8-weight proj_out cannot leave them
        p_out = None if self.fp8_linear else self._gn_tag(out, T, C, False)
        m = A.mark()
        g = A.alloc(R * T, C)
        o.groupnorm(x, g, R, T, w[path + ".norm.g"], w[path + ".norm.b"], 1e-6, False, self.cfg.norm_groups, self._gnws,
                    partials=self._gn_of(x))
        h = A.alloc(R * T, C)
        # LayerNorm folding needs every GEMM that writes h (K = C: proj_in, to_out; K = 4C: ff2) to leave the same partials layout
        lnst = None
        if self.ln_fold and depth > 0:
            parts = {ops.ln_parts(R * T, C, K) for K in (C, 4 * C)}
            if len(parts) == 1 and 0 not in parts:
                lnst = A.alloc(parts.pop() * R * T, 4).view(torch.float32).view(-1, R * T, 2)      # (parts, M, 2) fp32
        o.gemm(g, w[path + ".proj_in.w"], h, bias=w[path + ".proj_in.b"], ln_out=lnst)
        for k in range(depth):
            self._tblock(f"{path}.transformer_blocks.{k}", h, R, T, C // self.cfg.head_dim, st, ada, lnst, last=k == depth - 1,
                         grid=(H, W))
        o.gemm(h, w[path + ".proj_out.w"], out, bias=w[path + ".proj_out.b"], res=x, gn_out=p_out)
        A.release(m)
        return out

    def _embeddings(self, t_dev, st):
        """silu(emb) shared by every consumer, the batched time_emb_proj and adaLN GEMMs.
        emb = time_embedding(sincos(t)) + aug_emb (module/unet/unet_2d_ZeroSFT.py:1226-1243)."""
        o, w, A, cfg = self.o, self.w, self.arena, self.cfg
        R = st["R"]
        c0, td = cfg.block_out_channels[0], cfg.time_embed_dim
        sin = A.alloc(R, c0)
        o.sinusoid(t_dev, sin, c0)
        e1 = A.alloc(R, td)
        o.gemm(sin, w["time_embedding.linear_1.w"], e1, bias=w["time_embedding.linear_1.b"], act=ops.ACT_SILU)
        emb = A.alloc(R, td)
        o.gemm(e1, w["time_embedding.linear_2.w"], emb, bias=w["time_embedding.linear_2.b"], res=st["aug_emb"])
        act = A.alloc(R, td)
        o.silu(emb, act)
        temb_all = A.alloc(R, w["temb_all.w"].shape[0])
        o.gemm(act, w["temb_all.w"], temb_all, bias=w["temb_all.b"])
        ada = None
        if "ada_all.w" in w:
            ada = st["ada"]
            o.gemm(act, w["ada_all.w"], ada, bias=w["ada_all.b"])
            # AdaLayerNorm of every block's hoisted IP K / V in one launch (attention_processor.py:14-26,1173-1176)
            nip = cfg.num_ip_tokens
            o.adaln_batch(st["ada_jobs"], st["ada_njobs"], R * nip, max(cfg.block_out_channels), ada.stride(0), nip, nip,
                          (nip + 7) // 8 * 8)
        return temb_all, ada

    def _aug_emb(self, text_embeds, time_ids):
        """add_embedding(cat(pooled, sincos(time_ids))) -- step invariant."""
        cfg, w = self.cfg, self.w
        R = text_embeds.shape[0]
        a = torch.zeros(R, cfg.add_embed_in, dtype=F16, device=self.device)
        a[:, :cfg.pooled_dim] = text_embeds.to(self.device, F16)
        ops.sinusoid(time_ids.to(self.device, torch.float32).contiguous(), a, cfg.addition_time_embed_dim, col_off=cfg.pooled_dim)
        h = torch.empty(R, cfg.time_embed_dim, dtype=F16, device=self.device)
        ops.gemm(a, w["add_embedding.linear_1.w"], h, bias=w["add_embedding.linear_1.b"], act=ops.ACT_SILU)
        out = torch.empty(R, cfg.time_embed_dim, dtype=F16, device=self.device)
        ops.gemm(h, w["add_embedding.linear_2.w"], out, bias=w["add_embedding.linear_2.b"])
        return out

    def _down_and_mid(self, x, R, H, W, temb_all, ada, st):
        """conv_in output -> (mid output, skips with their (H, W)).  module/min_sdxl.py:620-677,757-779."""
        cfg, o, w, A = self.cfg, self.o, self.w, self.arena
        skips = [(x, H, W)]
        nb = len(cfg.block_out_channels)
        for i, c in enumerate(cfg.block_out_channels):
            for j in range(cfg.layers_per_block):
                x = self._resnet(f"down_blocks.{i}.resnets.{j}", x, R, H, W, temb_all)
                if cfg.transformer_depth[i] > 0:
                    x = self._transformer(f"down_blocks.{i}.attentions.{j}", x, cfg.transformer_depth[i], R, H, W, st, ada)
                skips.append((x, H, W))
            if i < nb - 1:
                p = f"down_blocks.{i}.downsamplers.0.conv"
                H2, W2 = (H + 1) // 2, (W + 1) // 2
                y = A.alloc(R * H2 * W2, c)
                o.conv2d(x.view(R, H, W, c), w[p + ".w"], y, stride=2, bias=w[p + ".b"], gn_out=self._gn_tag(y, H2 * W2, 9 * c, True))
                x, H, W = y, H2, W2
                skips.append((x, H, W))
        x = self._resnet("mid_block.resnets.0", x, R, H, W, temb_all)
        x = self._transformer("mid_block.attentions.0", x, cfg.mid_depth, R, H, W, st, ada)
        x = self._resnet("mid_block.resnets.1", x, R, H, W, temb_all)
        return x, H, W, skips


class _SegState:
    """What `_tblock` needs to perturb a selected attn1 the SEG way: the selected paths, the first perturbed batch row, and the
    Gaussian taps per axis extent as fp32 device vectors (`mean`: the sigma -> inf form, no taps)."""

    def __init__(self, paths, first, mean, taps):
        self.paths, self.first, self.mean, self.taps = frozenset(paths), int(first), bool(mean), taps


class HipUNet(_Net):
    """SDXL UNet with TA-IP cross-attention.  `lora`/`lora_scaling` build the previewer weight set."""

    def __init__(self, cfg: UNetConfig, sd: Dict[str, torch.Tensor], device, lora=None, lora_scaling=1.0, fp8_linear=False):
        if lora is not None:
            sd = _merge_lora({k: v.to(device) for k, v in sd.items()}, {k: v.to(device) for k, v in lora.items()}, lora_scaling)
        super().__init__(cfg, sd, True, device, fp8_linear=fp8_linear)
        skips = skip_channels(cfg)
        rev = list(reversed(cfg.block_out_channels))
        depth = list(reversed(cfg.transformer_depth))
        for i, c in enumerate(rev):
            for j in range(cfg.layers_per_block + 1):
                self._pack_resnet(sd, f"up_blocks.{i}.resnets.{j}", self._temb)
                if depth[i] > 0:
                    self._pack_transformer(sd, f"up_blocks.{i}.attentions.{j}", depth[i], self._ada)
            if i < len(rev) - 1:
                self._pack_conv3(sd, f"up_blocks.{i}.upsamplers.0.conv")
        self._pack_norm(sd, "conv_norm_out")
        self._pack_conv3(sd, "conv_out")
        self._finish_pack()
        self._pack_resampler(sd)
        self._sized = None
        # FreeU (module/min_sdxl.py:56-77): None, or (s1, s2, b1, b2) applied to the concats of up blocks 0 and 1
        self.freeu = None

    def set_pag(self, paths, ident_from):
        """Perturbed-attention guidance: in every `attn1` named in `paths`, the batch rows [ident_from, R) of a forward take the
        identity attention map (o = to_out(to_v(norm1(h)))); every other launch is unchanged.  `paths` None / empty: off.
        An engine built with fp8 linears is refused (ValueError)."""
        if not paths:
            self.pag = None
            return
        pag.check_engine(self)
        if int(ident_from) < 1:
            raise ValueError(f"set_pag: ident_from must be >= 1, got {ident_from}")
        self.pag = (frozenset(paths), int(ident_from))

    def set_seg(self, paths, first, sigma=seg.DEFAULT_SEG_BLUR_SIGMA, H=None, W=None):
        """Smoothed-energy guidance: in every `attn1` named in `paths`, the queries of the batch rows [first, R) of a forward on
        an H x W latent are blurred over the token grid with a Gaussian of `sigma` (`seg.weights`; beyond `seg.MEAN_ABOVE` the
        image's mean query) before a plain attention; every other launch is unchanged.  `paths` None / empty: off.  The taps
        of a (sigma, extent) pair are packed once and kept, so launches captured into a graph keep reading valid memory.
        An engine built with fp8 linears, PAG set on the same engine and a grid beyond `seg.MAX_EXTENT` are refused (ValueError)."""
        if not paths:
            self.seg = None
            return
        seg.check_engine(self)
        if self.pag is not None:
            raise ValueError("set_seg: perturbed-attention guidance is set on this UNet; both claim the perturbed rows")
        if int(first) < 1:
            raise ValueError(f"set_seg: first must be >= 1, got {first}")
        sigma = seg.check_sigma(sigma)
        seg.check_grids(self.cfg, paths, H, W)
        mean, taps = seg.is_mean(sigma), {}
        if not mean:
            cache = self.__dict__.setdefault("_seg_taps", {})
            for n in {n for hw in seg.level_grids(self.cfg, H, W) for n in hw}:
                if (sigma, n) not in cache:
                    cache[(sigma, n)] = torch.tensor(seg.weights(sigma, n), dtype=torch.float64).to(torch.float32).to(self.device)
                taps[n] = cache[(sigma, n)]
        self.seg = _SegState(paths, first, mean, taps)

    # ---- Resampler (runs once per image batch) ------------------------------------------------
    def _pack_resampler(self, sd):
        rc = self.cfg.resampler
        p = "encoder_hid_proj.image_projection_layers.0"
        self.w["rs.latents"] = self._t(sd, p + ".latents").reshape(rc.num_queries, rc.dim).contiguous()
        self._pack_linear(sd, p + ".proj_in", "rs.proj_in")
        self._pack_linear(sd, p + ".proj_out", "rs.proj_out")
        self._pack_norm(sd, p + ".norm_out")
        self.w["rs.norm_out.g"], self.w["rs.norm_out.b"] = self.w.pop(p + ".norm_out.g"), self.w.pop(p + ".norm_out.b")
        for i in range(rc.depth):
            a, f = f"{p}.layers.{i}.0", f"{p}.layers.{i}.1"
            for nn_ in ("norm1", "norm2"):
                self.w[f"rs.{i}.{nn_}.g"] = self._t(sd, f"{a}.{nn_}.weight").contiguous()
                self.w[f"rs.{i}.{nn_}.b"] = self._t(sd, f"{a}.{nn_}.bias").contiguous()
            self.w[f"rs.{i}.to_q.w"] = self._t(sd, a + ".to_q.weight").contiguous()
            self.w[f"rs.{i}.to_kv.w"] = self._t(sd, a + ".to_kv.weight").contiguous()
            self.w[f"rs.{i}.to_out.w"] = self._t(sd, a + ".to_out.weight").contiguous()
            self.w[f"rs.{i}.ffn.g"] = self._t(sd, f + ".0.weight").contiguous()
            self.w[f"rs.{i}.ffn.b"] = self._t(sd, f + ".0.bias").contiguous()
            self.w[f"rs.{i}.ff1.w"] = self._t(sd, f + ".1.weight").contiguous()
            self.w[f"rs.{i}.ff2.w"] = self._t(sd, f + ".3.weight").contiguous()

    def resampler(self, image_embeds: torch.Tensor) -> torch.Tensor:
        """(n, B, S, E) DINOv2 features -> (n*B, Q, D) IP tokens.  resampler.py:127-147, ip_adapter.py:81-86."""
        rc, w, dev = self.cfg.resampler, self.w, self.device
        x = image_embeds.to(dev, F16)
        Rr = x.shape[0] * x.shape[1]
        S = x.shape[2]
        x = x.reshape(Rr * S, x.shape[3]).contiguous()
        Q, D, inner, heads = rc.num_queries, rc.dim, rc.dim_head * rc.heads, rc.heads
        new = lambda r, c: torch.empty(r, c, dtype=F16, device=dev)
        xp = new(Rr * S, D)
        ops.gemm(x, w["rs.proj_in.w"], xp, bias=w["rs.proj_in.b"])
        lat = w["rs.latents"].repeat(Rr, 1).contiguous()                       # (Rr*Q, D)
        Tkv = S + Q
        tpad = (Tkv + 7) // 8 * 8
        cat = new(Rr * Tkv, D)
        cat3 = cat.view(Rr, Tkv, D)
        for i in range(rc.depth):
            # PerceiverAttention (resampler.py:50-78): kv input = cat(norm1(x), norm2(latents))
            for r in range(Rr):
                ops.layernorm(xp[r * S:(r + 1) * S], cat3[r, :S], w[f"rs.{i}.norm1.g"], w[f"rs.{i}.norm1.b"], 1e-5)
                ops.layernorm(lat[r * Q:(r + 1) * Q], cat3[r, S:], w[f"rs.{i}.norm2.g"], w[f"rs.{i}.norm2.b"], 1e-5)
            ln_lat = new(Rr * Q, D)
            ops.layernorm(lat, ln_lat, w[f"rs.{i}.norm2.g"], w[f"rs.{i}.norm2.b"], 1e-5)
            q = new(Rr * Q, inner)
            ops.gemm(ln_lat, w[f"rs.{i}.to_q.w"], q)
            kvb = new(Rr * Tkv, 2 * inner)
            ops.gemm(cat, w[f"rs.{i}.to_kv.w"], kvb)
            vt = torch.zeros(inner, Rr * tpad, dtype=F16, device=dev)
            for r in range(Rr):
                ops.transpose(kvb[r * Tkv:(r + 1) * Tkv, inner:], vt[:, r * tpad:(r + 1) * tpad], tpad)
            a = new(Rr * Q, inner)
            # (q d^-1/4)(k d^-1/4)^T = q k^T / sqrt(d); softmax in fp32 (resampler.py:72-74)
            ops.attention(q, a, [(kvb[:, :inner], Tkv, vt, tpad, Tkv)], Rr, heads, Q, scale=rc.dim_head ** -0.5)
            lat2 = new(Rr * Q, D)
            ops.gemm(a, w[f"rs.{i}.to_out.w"], lat2, res=lat)
            # FeedForward (resampler.py:13-20): LN, Linear, GELU, Linear, no biases
            h = new(Rr * Q, D)
            ops.layernorm(lat2, h, w[f"rs.{i}.ffn.g"], w[f"rs.{i}.ffn.b"], 1e-5)
            f = new(Rr * Q, D * rc.ff_mult)
            ops.gemm(h, w[f"rs.{i}.ff1.w"], f, act=ops.ACT_GELU)
            lat = new(Rr * Q, D)
            ops.gemm(f, w[f"rs.{i}.ff2.w"], lat, res=lat2)
        po = new(Rr * Q, rc.output_dim)
        ops.gemm(lat, w["rs.proj_out.w"], po, bias=w["rs.proj_out.b"])
        out = new(Rr * Q, rc.output_dim)
        ops.layernorm(po, out, w["rs.norm_out.g"], w["rs.norm_out.b"], 1e-5)
        return out.view(Rr, Q, rc.output_dim)

    # ---- per-batch preparation ----------------------------------------------------------------
    def prepare(self, ctx, text_embeds, time_ids, ip_tokens, H, W):
        """Hoist everything that does not depend on the step: aug_emb, text K / V^T and raw IP K / V
        projections of every cross-attention block.  ctx (R, L, Dc); ip_tokens (R, Q, Dc)."""
        cfg, w, dev = self.cfg, self.w, self.device
        R, L = ctx.shape[0], ctx.shape[1]
        assert L == cfg.text_len and ip_tokens.shape[1] == cfg.num_ip_tokens
        ctx2 = ctx.to(dev, F16).reshape(R * L, -1).contiguous()
        ip2 = ip_tokens.to(dev, F16).reshape(R * cfg.num_ip_tokens, -1).contiguous()
        tpad = (L + 7) // 8 * 8
        nip, ipad = cfg.num_ip_tokens, (cfg.num_ip_tokens + 7) // 8 * 8
        st = {"R": R, "H": H, "W": W, "aug_emb": self._aug_emb(text_embeds, time_ids), "kv": {}}
        blocks = sorted({k[: -len(".attn2.to_k.w")] for k in w if k.endswith(".attn2.to_k.w")})
        for p in blocks:
            C = w[p + ".attn2.to_k.w"].shape[0]
            tk = torch.empty(R * L, C, dtype=F16, device=dev)
            ops.gemm(ctx2, w[p + ".attn2.to_k.w"], tk)
            tv = torch.empty(R * L, C, dtype=F16, device=dev)
            ops.gemm(ctx2, w[p + ".attn2.to_v.w"], tv)
            tvt = torch.zeros(C, R * tpad, dtype=F16, device=dev)
            for r in range(R):
                ops.transpose(tv[r * L:(r + 1) * L], tvt[:, r * tpad:(r + 1) * tpad], tpad)
            ipk = torch.empty(R * cfg.num_ip_tokens, C, dtype=F16, device=dev)
            ops.gemm(ip2, w[p + ".attn2.processor.to_k_ip.w"], ipk)
            ipv = torch.empty(R * cfg.num_ip_tokens, C, dtype=F16, device=dev)
            ops.gemm(ip2, w[p + ".attn2.processor.to_v_ip.w"], ipv)
            st["kv"][p] = {"tk": tk, "tvt": tvt, "tpad": tpad, "ipk_raw": ipk, "ipv_raw": ipv,
                           "ipk": torch.zeros(R * nip, C, dtype=F16, device=dev), "ipvt": torch.zeros(C, R * ipad, dtype=F16, device=dev)}
        # per-step adaLN of the raw IP K / V: shift first, then scale (attention_processor.py:24); V is emitted transposed
        st["ada"] = torch.zeros(R, w["ada_all.w"].shape[0], dtype=F16, device=dev)
        jobs = []
        for p in blocks:
            kv, C = st["kv"][p], w[p + ".attn2.to_k.w"].shape[0]
            sk, sv = self._ada_slices[p + ".k"], self._ada_slices[p + ".v"]
            ada = st["ada"]
            jobs.append((kv["ipk_raw"], kv["ipk"], ada[:, sk.start:sk.start + C], ada[:, sk.start + C:sk.stop], False))
            jobs.append((kv["ipv_raw"], kv["ipvt"], ada[:, sv.start:sv.start + C], ada[:, sv.start + C:sv.stop], True))
        st["ada_jobs"], st["ada_njobs"] = ops.adaln_job_table(jobs, dev), len(jobs)
        key = (R, H, W, self.freeu is not None)          # FreeU partials take arena room: on / off is a different layout
        if self._sized != key:
            dummy = torch.empty(R * H * W, CPAD, dtype=F16, device="meta")
            self._size_arena(lambda: self._forward(dummy, None, st, None, None, None))
            self._sized = key
        return st

    # ---- forward ------------------------------------------------------------------------------
    def forward(self, sample, t_dev, st, down_res=None, mid_res=None, res_scale=None):
        """sample: (R*H*W, 64) fp16 NHWC latent (channels >= 4 zero).  t_dev: fp32 device tensor (R, 1).
        down_res: list of (R*h*w, C) tensors added to the skips; mid_res likewise; res_scale: fp32 device (R,)
        per-row scale of the residuals (cond_scale, pipelines/sdxl_instantir.py:1602-1603).
        Returns eps as an (R*H*W, 4) fp16 NHWC view into the arena (valid until the next forward)."""
        self._begin()
        return self._forward(sample, t_dev, st, down_res, mid_res, res_scale)

    def encode(self, sample, t_dev, st):
        """First half (embeddings, conv_in, down blocks, mid block): independent of the Aggregator residuals,
        so the caller may run it on a side stream while the previewer UNet / Aggregator run."""
        self._begin()
        return self._encode(sample, t_dev, st)

    def decode(self, enc, st, down_res=None, mid_res=None, res_scale=None, late_event=None):
        """Second half (residual adds, up blocks, conv_out) on the state returned by `encode`."""
        return self._decode(enc, st, down_res, mid_res, res_scale, late_event)

    def _forward(self, sample, t_dev, st, down_res, mid_res, res_scale):
        return self._decode(self._encode(sample, t_dev, st), st, down_res, mid_res, res_scale)

    def _encode(self, sample, t_dev, st):
        cfg, o, w, A = self.cfg, self.o, self.w, self.arena
        R, H, W = st["R"], st["H"], st["W"]
        temb_all, ada = self._embeddings(t_dev, st)
        x = A.alloc(R * H * W, cfg.block_out_channels[0])
        o.conv2d(sample.view(R, H, W, CPAD), w["conv_in.w"], x, bias=w["conv_in.b"], gn_out=self._gn_tag(x, H * W, 9 * CPAD, True))
        x, h, wd, skips = self._down_and_mid(x, R, H, W, temb_all, ada, st)
        return x, h, wd, skips, temb_all, ada

    def _decode(self, enc, st, down_res, mid_res, res_scale, late_event=None):
        """`late_event`: recorded on another stream once the residuals of the shallow skips are complete; the decoder waits
        for it only before up block 1 (the deep residuals it consumes first are already there)."""
        cfg, o, w, A = self.cfg, self.o, self.w, self.arena
        R = st["R"]
        x, h, wd, skips, temb_all, ada = enc
        skips = list(skips)
        rev = list(reversed(cfg.block_out_channels))
        depth = list(reversed(cfg.transformer_depth))
        nb = len(rev)
        pending_mid = mid_res            # added to the mid output when it is copied into the first concat
        for i, c in enumerate(rev):
            if late_event is not None and i == 1:
                torch.cuda.current_stream().wait_event(late_event)
            for j in range(cfg.layers_per_block + 1):
                sk, sh, sw = skips.pop()
                k = len(skips)           # index of this skip in push order
                cx, cs = x.shape[1], sk.shape[1]
                cat = A.alloc(R * h * wd, cx + cs)
                add = down_res[k] if down_res is not None else None
                if self.freeu is not None and i < 2:
                    # FreeU on the post-residual (hidden, skip) pair of up block i = resolution_idx
                    # (unet_2d_ZeroSFT_blocks.py:2600-2627): stats of the skip, then the concat with b / s applied
                    s_f, b_f = self.freeu[i], self.freeu[2 + i]
                    parts = A.alloc(R * ops.FREEU_SLABS * 7, 2 * cs).view(torch.float32)
                    o.freeu_stats(sk, parts, h, wd, add=add, add_scale=res_scale if add is not None else None)
                    o.freeu_concat(x, sk, cat, parts, h, wd, b_f, s_f, mid_add=pending_mid, add=add,
                                   add_scale=res_scale if (add is not None or pending_mid is not None) else None)
                    pending_mid = None
                else:
                    # torch.cat([hidden, skip], dim=1) (module/min_sdxl.py:712) written in place; ControlNet
                    # residuals (stock diffusers: skip + residual) folded into the copies.
                    o.copy_add(x, cat, 0, add=pending_mid, add_scale=res_scale if pending_mid is not None else None,
                               rows_per_scale=h * wd)
                    pending_mid = None
                    o.copy_add(sk, cat, cx, add=add, add_scale=res_scale if down_res is not None else None,
                               rows_per_scale=h * wd)
                x = self._resnet(f"up_blocks.{i}.resnets.{j}", cat, R, h, wd, temb_all)
                if depth[i] > 0:
                    x = self._transformer(f"up_blocks.{i}.attentions.{j}", x, depth[i], R, h, wd, st, ada)
            if i < nb - 1:
                p = f"up_blocks.{i}.upsamplers.0.conv"
                y = A.alloc(R * 4 * h * wd, c)
                o.conv2d(x.view(R, h, wd, c), w[p + ".w"], y, upsample=True, bias=w[p + ".b"])
                x, h, wd = y, 2 * h, 2 * wd
        c0 = cfg.block_out_channels[0]
        g = A.alloc(R * h * wd, c0)
        o.groupnorm(x, g, R, h * wd, w["conv_norm_out.g"], w["conv_norm_out.b"], 1e-5, True, cfg.norm_groups, self._gnws,
                    partials=self._gn_of(x))
        eps = A.alloc(R * h * wd, cfg.out_channels)
        o.conv2d(g.view(R, h, wd, c0), w["conv_out.w"], eps, bias=w["conv_out.b"])
        return eps


class HipAggregator(_Net):
    """Aggregator: SDXL encoder half on the (2H x W) concat of LQ latent and preview, SFT heads."""

    def __init__(self, cfg: UNetConfig, sd: Dict[str, torch.Tensor], device):
        super().__init__(cfg, sd, False, device)
        self.defer_shallow = False
        self._late = []
        self._pack_conv3(sd, "ref_conv_in", CPAD)
        names = [f"controlnet_down_blocks.{k}" for k in range(len(skip_channels(cfg)))] + ["controlnet_mid_block"]
        for p in names:
            w0 = conv_weight_nhwc(self._t(sd, p + ".0.mlp_shared.0.weight"))
            self.w[p + ".shared.w"], self.w[p + ".shared.b"] = w0, self._t(sd, p + ".0.mlp_shared.0.bias").contiguous()
            wm, wa = conv_weight_nhwc(self._t(sd, p + ".0.mul.weight")), conv_weight_nhwc(self._t(sd, p + ".0.add.weight"))
            self.w[p + ".ga.w"] = pair_rows(wm, wa)                       # gamma rows | beta rows
            self.w[p + ".ga.b"] = pair_rows(self._t(sd, p + ".0.mul.bias"), self._t(sd, p + ".0.add.bias"))
            w1 = self._t(sd, p + ".1.weight")
            self.w[p + ".zero.w"] = w1.reshape(w1.shape[0], w1.shape[1]).contiguous()
            self.w[p + ".zero.b"] = self._t(sd, p + ".1.bias").contiguous()
        self._finish_pack()
        self._sized = None
        self._out: Optional[List[torch.Tensor]] = None

    def prepare(self, text_embeds, time_ids, H, W, out_rows=None):
        """`out_rows` (>= R): images the residual buffers hold.  The forward writes the first R; perturbed-attention guidance
        fills the rest with the cond rows' residuals (one batched copy, see pipeline._DenoiseLoop)."""
        R = text_embeds.shape[0]
        st = {"R": R, "H": H, "W": W, "aug_emb": self._aug_emb(text_embeds, time_ids), "kv": {}}
        Ro = R if out_rows is None else int(out_rows)
        assert Ro >= R
        key = (R, H, W) if Ro == R else (R, H, W, Ro)
        if self._sized != key:
            # residual outputs live outside the arena: they are consumed by the following UNet forward
            cfgc = skip_channels(self.cfg)
            hs, h, wd = [], H, W
            hs.append((h, wd))
            for i in range(len(self.cfg.block_out_channels)):
                hs += [(h, wd)] * self.cfg.layers_per_block
                if i < len(self.cfg.block_out_channels) - 1:
                    h, wd = (h + 1) // 2, (wd + 1) // 2
                    hs.append((h, wd))
            self._out = [torch.empty(Ro * a * b, c, dtype=F16, device=self.device) for (a, b), c in zip(hs, cfgc)]
            self._out_mid = torch.empty(Ro * h * wd, self.cfg.block_out_channels[-1], dtype=F16, device=self.device)
            dummy = torch.empty(R * H * W, CPAD, dtype=F16, device="meta")
            self._size_arena(lambda: self._forward(dummy, dummy, None, st))
            self._sized = key
        return st

    def forward(self, lq, preview, t_dev, st):
        """lq, preview: (R*H*W, 64) fp16 NHWC latents.  Returns (list of 9 residuals, mid residual),
        each (R*h*w, C) fp16 NHWC, un-scaled (conditioning_scale = 1, module/aggregator.py:963-964)."""
        self._begin()
        return self._forward(lq, preview, t_dev, st)

    def _sft(self, p, s, R, h2, wd, out):
        """SFT + zero 1x1 on a (R, 2h, w, C) map: cond = top half, h = bottom half.
        module/aggregator.py:940-948, :76-86."""
        self._unit(p)
        o, w, A, cfg = self.o, self.w, self.arena, self.cfg
        C = s.shape[1]
        h = h2 // 2
        m = A.mark()
        s4 = s.view(R, h2, wd, C)
        actv = A.alloc(R * h * wd, cfg.sft_hidden)
        o.conv2d(s4[:, :h], w[p + ".shared.w"], actv, bias=w[p + ".shared.b"], act=ops.ACT_SILU)
        mod = A.alloc(R * h * wd, C)
        ref = s[h * wd:]                                   # row 0 of image 0's bottom half; image stride 2*h*w rows
        o.conv2d(actv.view(R, h, wd, cfg.sft_hidden), w[p + ".ga.w"], mod, bias=w[p + ".ga.b"], res=ref, epi=ops.EPI_SFT,
                 res_img_rows=h2 * wd)
        o.gemm(mod, w[p + ".zero.w"], out[:R * h * wd], bias=w[p + ".zero.b"])
        A.release(m)

    def _forward(self, lq, preview, t_dev, st):
        cfg, o, w, A = self.cfg, self.o, self.w, self.arena
        R, H, W = st["R"], st["H"], st["W"]
        temb_all, ada = self._embeddings(t_dev, st)
        c0 = cfg.block_out_channels[0]
        x = A.alloc(R * 2 * H * W, c0)
        # torch.cat([conv_in(lq), ref_conv_in(preview)], dim=-2)  (module/aggregator.py:889-902)
        o.conv2d(lq.view(R, H, W, CPAD), w["conv_in.w"], x, bias=w["conv_in.b"], y_img_rows=2 * H * W)
        o.conv2d(preview.view(R, H, W, CPAD), w["ref_conv_in.w"], x[H * W:], bias=w["ref_conv_in.b"], y_img_rows=2 * H * W)
        xm, h2, wd, skips = self._down_and_mid(x, R, 2 * H, W, temb_all, ada, st)
        # heads in the order the UNet decoder consumes their residuals: mid, then the deepest skips.  With `defer_shallow`
        # the heads of the skips used by the LAST two up blocks are left to `late_heads()` (the caller runs it on another
        # stream, beside the decoder's first up block).
        self._sft("controlnet_mid_block", xm, R, h2, wd, self._out_mid)
        n_deep = cfg.layers_per_block + 1                       # skips popped by up block 0
        self._late = []
        for k in reversed(range(len(skips))):
            s, sh, sw = skips[k]
            if self.defer_shallow and k < len(skips) - n_deep:
                self._late.append((k, s, sh, sw))
            else:
                self._sft(f"controlnet_down_blocks.{k}", s, R, sh, sw, self._out[k])
        self._late_R = R
        return self._out, self._out_mid

    def late_heads(self):
        for k, s, sh, sw in self._late:
            self._sft(f"controlnet_down_blocks.{k}", s, self._late_R, sh, sw, self._out[k])
        self._late = []
