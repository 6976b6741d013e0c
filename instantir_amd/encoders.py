"""Image / text encoders that feed the denoising loop once per batch, on the same HIP kernels.

* `HipDinov2`: the DINOv2 ViT the reference loads with `AutoModel.from_pretrained(dinov2)`
  (`module/ip_adapter/utils.py:106-118`) and runs in `encode_image` on the image AND on `zeros_like(image)`
  (`pipelines/sdxl_instantir.py:660-667`), returning `last_hidden_state` (B, 257, 1024 @ 224 px).
  Architecture = transformers `Dinov2Model` (third-party, `transformers==4.36.2` pinned by requirements.txt:2):
  14x14/14 patch conv + CLS + bicubic-resized position table, pre-LN blocks (MHA with biases, LayerScale, GELU
  MLP), final LayerNorm.  Parameter names are the Hugging Face ones.
* `HipCLIPVision`: the CLIP vision tower of the `use_clip_encoder` branch, same kernels and padding.  Head dims 64
  (ViT-B / ViT-L), 80 (OpenCLIP ViT-H/14) and 104 (OpenCLIP ViT-bigG/14); other head dims are refused.
* `HipCLIPText`: the two CLIP text transformers of `encode_prompt`, causal attention over 77 -> 80 rows.

The three towers share one pre-LN transformer block, defined once: `_pack_blocks` packs its weights from a per-architecture
map of parameter names (`DINOV2_BLOCK`, `CLIP_BLOCK`), `_run_blocks` launches it.  MI355X mapping: tokens of a sequence are
padded to a multiple of 8 rows (257 -> 264) so every matrix keeps the alignment the kernels want; pad rows are computed and
ignored (keys beyond 257 are masked in the attention kernel).  LayerScale is folded into the output projections
(W' = diag(lambda) W), the value bias into the projection bias (softmax rows sum to 1: (P(V + 1 b^T)) Wo^T = (P V) Wo^T + Wo b),
Q|K are one GEMM, V is produced transposed by swapping GEMM operands.  The two image towers also share the patch-embedding
prologue and `encode_image_pair` (`_VisionTower`): the zero-image branch is input independent and cached per geometry
(SURVEY.md Appendix C Q7).  `_project_rows` is the pooled-feature projection of `image_embeds` and `text_embeds`.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import ops

F16 = torch.float16
CLIP_VISION_HEAD_DIMS = (64, 80, 104)      # head dims with an attention kernel (iir_attention_d64_f16, iir_attention_f16)
ACTS = {"quick_gelu": ops.ACT_QUICKGELU, "gelu": ops.ACT_GELU}

# Hugging Face parameter names of one pre-LN block, below "<layers><i>."; `mlp.fc1` / `mlp.fc2` are common to both
DINOV2_BLOCK = dict(layers="encoder.layer.", n1="norm1", n2="norm2", q="attention.attention.query", k="attention.attention.key",
                    v="attention.attention.value", o="attention.output.dense", ls=("layer_scale1.lambda1", "layer_scale2.lambda1"))
CLIP_BLOCK = dict(layers="encoder.layers.", n1="layer_norm1", n2="layer_norm2", q="self_attn.q_proj", k="self_attn.k_proj",
                  v="self_attn.v_proj", o="self_attn.out_proj", ls=None)


def _reader(sd, dev, prefix=""):
    """(sd without `prefix` on its keys, name -> that parameter in fp32 on `dev`)"""
    sd = {(k[len(prefix):] if prefix and k.startswith(prefix) else k): v for k, v in sd.items()}
    return sd, lambda n: sd[n].to(dev, torch.float32)


def _pack_blocks(sd, f32, w, names) -> int:
    """Pack every pre-LN block of `sd` into `w` ("<i>.n1.g" ... "<i>.fc2.b", fp16) and return the depth, read from the keys."""
    depth = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith(names["layers"]))
    h = lambda t: t.to(F16).contiguous()
    for i in range(depth):
        p = f"{names['layers']}{i}."
        for n in ("n1", "n2"):
            w[f"{i}.{n}.g"], w[f"{i}.{n}.b"] = h(f32(p + names[n] + ".weight")), h(f32(p + names[n] + ".bias"))
        w[f"{i}.qk.w"] = h(torch.cat([f32(p + names["q"] + ".weight"), f32(p + names["k"] + ".weight")]))
        w[f"{i}.qk.b"] = h(torch.cat([f32(p + names["q"] + ".bias"), f32(p + names["k"] + ".bias")]))
        w[f"{i}.v.w"] = h(f32(p + names["v"] + ".weight"))
        wo = f32(p + names["o"] + ".weight")
        bo = wo @ f32(p + names["v"] + ".bias") + f32(p + names["o"] + ".bias")         # value bias folded
        w2, b2 = f32(p + "mlp.fc2.weight"), f32(p + "mlp.fc2.bias")
        if names["ls"]:                                                                # LayerScale folded
            ls1, ls2 = f32(p + names["ls"][0]), f32(p + names["ls"][1])
            wo, bo, w2, b2 = ls1[:, None] * wo, ls1 * bo, ls2[:, None] * w2, ls2 * b2
        w[f"{i}.o.w"], w[f"{i}.o.b"], w[f"{i}.fc2.w"], w[f"{i}.fc2.b"] = h(wo), h(bo), h(w2), h(b2)
        w[f"{i}.fc1.w"], w[f"{i}.fc1.b"] = h(f32(p + "mlp.fc1.weight")), h(f32(p + "mlp.fc1.bias"))
    return depth


def _run_blocks(w, h, n_layers, B, Tp, T, heads, head_dim, act, eps, causal=False, keep=None):
    """Run blocks [0, n_layers) on h (B * Tp rows, the first T of every Tp real) in place.  Returns a clone of h taken before
    block `keep` (None when that block is not run): `hidden_states[keep]`."""
    M, D = h.shape
    n = torch.empty(M, D, dtype=F16, device=h.device)
    qk = torch.empty(M, 2 * D, dtype=F16, device=h.device)
    vt = torch.empty(D, M, dtype=F16, device=h.device)
    a = torch.empty(M, D, dtype=F16, device=h.device)
    f = torch.empty(M, w["0.fc1.w"].shape[0], dtype=F16, device=h.device)
    kept = None
    for i in range(n_layers):
        if i == keep:
            kept = h.clone()
        ops.layernorm(h, n, w[f"{i}.n1.g"], w[f"{i}.n1.b"], eps)
        ops.gemm(n, w[f"{i}.qk.w"], qk, bias=w[f"{i}.qk.b"])
        ops.gemm(w[f"{i}.v.w"], n, vt)                                   # V^T (value bias folded into o.b)
        ops.attention(qk[:, :D], a, [(qk[:, D:], Tp, vt, Tp, T)], B, heads, Tp, scale=head_dim ** -0.5, causal=causal,
                      head_dim=head_dim)
        ops.gemm(a, w[f"{i}.o.w"], h, bias=w[f"{i}.o.b"], res=h)
        ops.layernorm(h, n, w[f"{i}.n2.g"], w[f"{i}.n2.b"], eps)
        ops.gemm(n, w[f"{i}.fc1.w"], f, bias=w[f"{i}.fc1.b"], act=act)
        ops.gemm(f, w[f"{i}.fc2.w"], h, bias=w[f"{i}.fc2.b"], res=h)
    return kept


def _project_rows(rows, proj, norm=None, eps=None):
    """rows (B, D) -> (B, P) through `proj` (P, D, no bias), after a LayerNorm `norm` = (gamma, beta) if given; B is padded
    to a multiple of 8 rows for the GEMM."""
    B = rows.shape[0]
    rows8 = torch.zeros((B + 7) // 8 * 8, rows.shape[1], dtype=F16, device=rows.device)
    rows8[:B] = rows
    if norm is not None:
        rows8 = ops.layernorm(rows8, torch.empty_like(rows8), norm[0], norm[1], eps)
    out = torch.empty(rows8.shape[0], proj.shape[0], dtype=F16, device=rows.device)
    ops.gemm(rows8, proj, out)
    return out[:B]


class _VisionTower:
    """What the two ViT image towers share: the patch-embedding prologue and `encode_image_pair`.  A tower supplies
    `_pos_rows(H, W, gh, gw)` -> (position rows of the patches, CLS token + its position row) and `forward`."""

    def _pack_patch(self, wp):
        """wp (D, 3, p, p): starts `w` with the patch conv as a (D, 3 p p) GEMM weight, zero-padded to a K tile multiple."""
        self.D, kp = wp.shape[0], wp[0].numel()
        self.kpad = (kp + 63) // 64 * 64
        self.w = {"patch.w": torch.nn.functional.pad(wp.reshape(self.D, kp), (0, self.kpad - kp)).to(F16).contiguous()}
        self._zero_cache = {}

    def _embed(self, pixel_values):
        """Token rows before the first block: (e (B * Tp, D) with zero pad rows, B, T, Tp)."""
        dev, D, ps, w = self.device, self.D, self.patch, self.w
        x = pixel_values.to(dev, torch.float32)
        B, _, H, W = x.shape
        gh, gw = H // ps, W // ps
        T = 1 + gh * gw
        Tp = (T + 7) // 8 * 8
        pos_patch, cls_row = self._pos_rows(H, W, gh, gw)
        # patchify (pure data movement): (B, 3, gh, p, gw, p) -> (B*gh*gw, 3*p*p) zero-padded to a K tile multiple
        pt = x[:, :, :gh * ps, :gw * ps].reshape(B, 3, gh, ps, gw, ps).permute(0, 2, 4, 1, 3, 5).reshape(B * gh * gw, 3 * ps * ps)
        patches = torch.zeros(B * gh * gw, self.kpad, dtype=F16, device=dev)
        patches[:, :3 * ps * ps] = pt.to(F16)
        e = torch.zeros(B * Tp, D, dtype=F16, device=dev)
        e3 = e.view(B, Tp, D)
        e3[:, 0] = cls_row                                               # CLS token + its position row (constants)
        for b in range(B):                                              # patch projection (+ bias) + position rows
            ops.gemm(patches[b * gh * gw:(b + 1) * gh * gw], w["patch.w"], e3[b, 1:T], bias=w.get("patch.b"), res=pos_patch)
        return e, B, T, Tp

    def encode_image_pair(self, pixel_values: torch.Tensor):
        """`encode_image` (pipelines/sdxl_instantir.py:660-667 for DINOv2, :644-654 with `output_hidden_states=True` for
        CLIP): features of the image and of `zeros_like(image)`; the latter depends only on the geometry and is cached."""
        feats = self.forward(pixel_values)
        key = tuple(pixel_values.shape[1:])
        if key not in self._zero_cache:
            self._zero_cache[key] = self.forward(torch.zeros(1, *key))
        return feats, self._zero_cache[key].expand(pixel_values.shape[0], -1, -1)


class HipDinov2(_VisionTower):
    def __init__(self, sd: Dict[str, torch.Tensor], device, patch_size=14, num_heads=None, eps=1e-6):
        self.device = torch.device(device)
        sd, f32 = _reader(sd, self.device)
        self.patch = patch_size
        self._pack_patch(f32("embeddings.patch_embeddings.projection.weight"))   # (D, 3, p, p)
        D = self.D
        self.heads = num_heads if num_heads is not None else D // 64
        if D // self.heads != 64:
            raise ValueError("HipDinov2 uses the head_dim-64 attention kernel (ViT-S/B/L/g all have 64)")
        self.w["patch.b"] = f32("embeddings.patch_embeddings.projection.bias").to(F16)
        self.cls = f32("embeddings.cls_token").reshape(D)
        self.pos = f32("embeddings.position_embeddings")                      # (1, 1 + n^2, D)
        self.eps = eps
        self.depth = _pack_blocks(sd, f32, self.w, DINOV2_BLOCK)
        self.w["ln.g"], self.w["ln.b"] = f32("layernorm.weight").to(F16), f32("layernorm.bias").to(F16)
        self._pos_cache = {}

    def _pos_rows(self, H, W, gh, gw):
        """Position table for a gh x gw patch grid: bicubic resize of the stored square table (one-time weight
        preprocessing, same call as transformers' Dinov2Embeddings.interpolate_pos_encoding)."""
        key = (gh, gw)
        if key not in self._pos_cache:
            n = self.pos.shape[1] - 1
            side = int(round(n ** 0.5))
            if gh * gw == n and gh == gw:
                table = self.pos[0]
            else:
                pp = self.pos[:, 1:].reshape(1, side, side, self.D).permute(0, 3, 1, 2)
                pp = torch.nn.functional.interpolate(pp, size=(gh, gw), mode="bicubic", align_corners=False)
                table = torch.cat([self.pos[0, :1], pp.permute(0, 2, 3, 1).reshape(gh * gw, self.D)])
            self._pos_cache[key] = (table[1:].to(F16).contiguous(), (self.cls + table[0]).to(F16))
        return self._pos_cache[key]

    @torch.no_grad()
    def forward(self, pixel_values: torch.Tensor) -> torch.Tensor:
        """pixel_values (B, 3, H, W), already normalised (AutoImageProcessor).  Returns last_hidden_state
        (B, 1 + (H/14)(W/14), D) fp16."""
        h, B, T, Tp = self._embed(pixel_values)
        _run_blocks(self.w, h, self.depth, B, Tp, T, self.heads, 64, ops.ACT_GELU, self.eps)
        n = ops.layernorm(h, torch.empty_like(h), self.w["ln.g"], self.w["ln.b"], self.eps)
        return n.view(B, Tp, self.D)[:, :T]

    __call__ = forward


def _preprocess_geometry(w0, h0, size, crop):
    """(resized (H, W), crop window (top, left, crop, crop)) of the image processors: shortest edge to `size`, centre crop."""
    s = size / min(w0, h0)
    nw, nh = max(crop, round(w0 * s)), max(crop, round(h0 * s))
    return (nh, nw), ((nh - crop) // 2, (nw - crop) // 2, crop, crop)


def _preprocess_device(images, size, crop, mean, std, device):
    """The image processors on the device: one uint8 upload per image size, a bicubic resize in quantised mode (what PIL does to
    an 8-bit image) with the centre crop as the launch's window and rescale + normalise as its per-channel affine
    (v / (255 std) - mean / std).  PIL image(s), or a tensor of 0..255-valued pixels ((N, 3, H, W) float or (N, H, W, 3) uint8)."""
    from . import resample as RS
    scale, bias = tuple(1.0 / (255.0 * s) for s in std), tuple(-m / s for m, s in zip(mean, std))
    if torch.is_tensor(images):
        groups = [images]
    else:
        groups = [im.convert("RGB") for im in (images if isinstance(images, (list, tuple)) else [images])]
        if len({im.size for im in groups}) == 1:
            groups = [groups]                                            # one size: one upload, one launch pair
    out = []
    for g in groups:
        batch, kind = RS.as_batch(g)
        h0, w0 = batch.shape[1:3] if kind == "u8" else batch.shape[2:4]
        full, window = _preprocess_geometry(w0, h0, size, crop)
        out.append(RS.resize_images(batch, full, "bicubic", device, quantize=True, window=window, scale=scale, bias=bias))
    return out[0] if len(out) == 1 else torch.cat(out)


def dinov2_preprocess(images, size=256, crop=224, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), device=None):
    """AutoImageProcessor of facebook/dinov2-* (BitImageProcessor): bicubic resize of the shortest edge to 256,
    centre crop 224, rescale 1/255, ImageNet normalise (SURVEY.md Appendix A "Image I/O").  PIL in, fp32 NCHW out.
    With a `device` the same steps run there (`_preprocess_device`; a tensor of 0..255-valued pixels is accepted as well) and
    the result stays on it; at most 1 LSB from the host form before normalisation."""
    if device is not None:
        return _preprocess_device(images, size, crop, mean, std, device)
    if torch.is_tensor(images):
        raise ValueError("a tensor as the raw image needs `device=`: the host form takes PIL images")
    import numpy as np
    from PIL import Image
    out = []
    for im in images if isinstance(images, (list, tuple)) else [images]:
        im = im.convert("RGB")
        w0, h0 = im.size
        s = size / min(w0, h0)
        im = im.resize((max(crop, round(w0 * s)), max(crop, round(h0 * s))), Image.BICUBIC)
        l, t = (im.size[0] - crop) // 2, (im.size[1] - crop) // 2
        arr = np.asarray(im.crop((l, t, l + crop, t + crop)), dtype=np.float32) / 255.0
        out.append((arr - np.array(mean, dtype=np.float32)) / np.array(std, dtype=np.float32))
    return torch.from_numpy(np.stack(out)).permute(0, 3, 1, 2).contiguous()


def clip_preprocess(images, size=224, mean=(0.48145466, 0.4578275, 0.40821073), std=(0.26862954, 0.26130258, 0.27577711), device=None):
    """`CLIPImageProcessor()` with its defaults (module/ip_adapter/utils.py:114-118): bicubic resize of the shortest edge to
    224, centre crop 224, rescale 1/255, CLIP normalise.  PIL in, fp32 NCHW out; `device`: as for `dinov2_preprocess`."""
    return dinov2_preprocess(images, size=size, crop=size, mean=mean, std=std, device=device)


class HipCLIPVision(_VisionTower):
    """CLIP vision tower (transformers `CLIPVisionModelWithProjection`, third-party) for the reference's `use_clip_encoder`
    branch (`module/ip_adapter/utils.py:106-118`).  With a Resampler as the image projector the pipeline asks for
    `hidden_states[-2]` of the image and of `zeros_like(image)` (`pipelines/sdxl_instantir.py:696-699,644-654`); `image_embeds`
    (post-LayerNorm CLS feature through `visual_projection`) is provided as well (:656-659).

    Patch conv without bias + class embedding + learned position table (fixed geometry), `pre_layrnorm` (sic, the HF
    parameter name), pre-LN blocks with unmasked attention, quick-GELU or GELU MLP.  Token rows are padded to a multiple
    of 8 (257 -> 264, pad keys masked).  Head dims 64 (ViT-B/16, ViT-B/32, ViT-L/14: `iir_attention_d64_f16`), 80
    (OpenCLIP ViT-H/14) and 104 (OpenCLIP ViT-bigG/14; both `iir_attention_f16`); every other head dim is refused with a
    ValueError.  `num_heads` / `hidden_act` / `eps` must come from the tower's config: D // 64 heads is only a default."""

    def __init__(self, sd: Dict[str, torch.Tensor], device, patch_size=None, num_heads=None, eps=1e-5, hidden_act="quick_gelu"):
        self.device = torch.device(device)
        sd, f32 = _reader(sd, self.device, "vision_model.")
        wp = f32("embeddings.patch_embedding.weight")                    # (D, 3, p, p), no bias
        D = wp.shape[0]
        self.patch = wp.shape[-1] if patch_size is None else patch_size
        self.heads = num_heads if num_heads is not None else D // 64
        self.head_dim = D // self.heads
        if D % self.heads or self.head_dim not in CLIP_VISION_HEAD_DIMS:
            raise ValueError(f"HipCLIPVision: {D} features in {self.heads} heads -- the attention kernels take head dims "
                             f"{CLIP_VISION_HEAD_DIMS} (CLIP ViT-B / ViT-L, ViT-H/14, ViT-bigG/14) only")
        self._pack_patch(wp)
        self.act = ACTS[hidden_act]
        self.eps = eps
        w = self.w
        pos = f32("embeddings.position_embedding.weight")                # (1 + n^2, D)
        self.n_pos = pos.shape[0]
        w["pos"] = pos[1:].to(F16).contiguous()
        w["cls"] = (f32("embeddings.class_embedding").reshape(D) + pos[0]).to(F16)
        w["pre.g"], w["pre.b"] = f32("pre_layrnorm.weight").to(F16), f32("pre_layrnorm.bias").to(F16)
        self.depth = _pack_blocks(sd, f32, w, CLIP_BLOCK)
        w["post.g"], w["post.b"] = f32("post_layernorm.weight").to(F16), f32("post_layernorm.bias").to(F16)
        self.proj = sd["visual_projection.weight"].to(self.device, F16).contiguous() if "visual_projection.weight" in sd else None

    def _pos_rows(self, H, W, gh, gw):
        if 1 + gh * gw != self.n_pos:
            raise ValueError(f"CLIP vision tower has a fixed position table of {self.n_pos} tokens; a {H}x{W} input gives {1 + gh * gw}")
        return self.w["pos"], self.w["cls"]

    @torch.no_grad()
    def forward(self, pixel_values: torch.Tensor, with_embeds: bool = False):
        """pixel_values (B, 3, H, W) normalised (CLIPImageProcessor).  Returns hidden_states[-2] (B, 1 + (H/p)(W/p), D) fp16
        [and image_embeds (B, P) when `with_embeds`]."""
        w, D = self.w, self.D
        e, B, T, Tp = self._embed(pixel_values)
        h = ops.layernorm(e, torch.empty_like(e), w["pre.g"], w["pre.b"], self.eps)      # hidden_states[0]
        # hidden_states[-2] is the INPUT of the last layer, which only image_embeds need
        penult = _run_blocks(w, h, self.depth if with_embeds else self.depth - 1, B, Tp, T, self.heads, self.head_dim, self.act,
                             self.eps, keep=self.depth - 1)
        if not with_embeds:
            return h.view(B, Tp, D)[:, :T]
        if self.proj is None:
            raise ValueError("image_embeds need `visual_projection.weight` (a CLIPVisionModelWithProjection state dict)")
        embeds = _project_rows(h.view(B, Tp, D)[:, 0], self.proj, (w["post.g"], w["post.b"]), self.eps)     # pooled = CLS row
        return penult.view(B, Tp, D)[:, :T], embeds

    __call__ = forward


class HipCLIPText:
    """CLIP text transformer (transformers `CLIPTextModel` / `CLIPTextModelWithProjection`, third-party) as used by
    `encode_prompt` (pipelines/sdxl_instantir.py:400-632): SDXL takes `hidden_states[-2]` of both encoders (768 + 1280
    features, concatenated to the 2048-wide context) and the projected EOS feature of the second one (`text_embeds`).

    Pre-LN blocks with causal self-attention (heads of dim 64: 12 for CLIP-L, 20 for OpenCLIP-bigG), quick-GELU or GELU
    MLP.  Sequences are padded from 77 to 80 rows; the causal mask also hides the pad keys from every real query."""

    def __init__(self, sd: Dict[str, torch.Tensor], device, hidden_act="quick_gelu", eos_token_id=2, eps=1e-5):
        self.device = torch.device(device)
        sd, f32 = _reader(sd, self.device, "text_model.")
        self.tok = f32("embeddings.token_embedding.weight").to(F16)
        self.pos = f32("embeddings.position_embedding.weight").to(F16)
        self.D = D = self.tok.shape[1]
        self.heads = D // 64
        self.act = ACTS[hidden_act]
        self.eos_token_id, self.eps = eos_token_id, eps
        self.w = {}
        self.depth = _pack_blocks(sd, f32, self.w, CLIP_BLOCK)
        self.w["ln.g"], self.w["ln.b"] = f32("final_layer_norm.weight").to(F16), f32("final_layer_norm.bias").to(F16)
        self.proj = sd["text_projection.weight"].to(self.device, F16).contiguous() if "text_projection.weight" in sd else None

    @torch.no_grad()
    def forward(self, input_ids: torch.Tensor, clip_skip=None):
        """input_ids (B, T<=77) int64.  Returns (hidden_states[-2] (B, T, D) fp16 -- hidden_states[-(clip_skip + 2)] when
        `clip_skip` is given, pipelines/sdxl_instantir.py:524-530 -- and text_embeds (B, P) fp16 or None)."""
        take = self.depth - 1 - (clip_skip or 0)            # the kept state is the INPUT of layer `take`
        if not 0 <= take < self.depth:
            raise ValueError(f"clip_skip={clip_skip} out of range for a {self.depth}-layer text encoder")
        dev, D, w = self.device, self.D, self.w
        ids = input_ids.to(dev)
        B, T = ids.shape
        Tp = (T + 7) // 8 * 8
        M = B * Tp
        emb = torch.zeros(M, D, dtype=F16, device=dev)
        emb.view(B, Tp, D)[:, :T] = self.tok[ids]                        # gather (data movement)
        pos = torch.zeros(M, D, dtype=F16, device=dev)
        pos.view(B, Tp, D)[:, :T] = self.pos[:T]
        h = torch.empty(M, D, dtype=F16, device=dev)
        ops.copy_add(emb, h, 0, add=pos)                                  # token + position embeddings
        penult = _run_blocks(w, h, self.depth, B, Tp, T, self.heads, 64, self.act, self.eps, causal=True, keep=take)
        pooled = None
        if self.proj is not None:
            n = ops.layernorm(h, torch.empty_like(h), w["ln.g"], w["ln.b"], self.eps)    # final_layer_norm
            if self.eos_token_id == 2:                                    # legacy configs: eot = highest id in the sequence
                eos = ids.to(torch.int).argmax(dim=-1)
            else:
                eos = (ids == self.eos_token_id).int().argmax(dim=-1)
            pooled = _project_rows(n.view(B, Tp, D)[torch.arange(B, device=dev), eos], self.proj)     # text_projection
        return penult.view(B, Tp, D)[:, :T], pooled

    __call__ = forward


def encode_prompt_ids(enc1: HipCLIPText, enc2: HipCLIPText, ids1: torch.Tensor, ids2: torch.Tensor, clip_skip=None):
    """The tensor part of `encode_prompt` (pipelines/sdxl_instantir.py:516-560): concat the two penultimate hidden
    states -> (B, 77, 2048) prompt_embeds; pooled = projected EOS feature of the second encoder -> (B, 1280)."""
    h1, _ = enc1(ids1, clip_skip)
    h2, pooled = enc2(ids2, clip_skip)
    return torch.cat([h1, h2], dim=-1), pooled
