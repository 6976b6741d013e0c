"""Head-dim 80 / 104 attention (iir_attention_f16) at the CLIP ViT-H/14 and bigG/14 tower shapes, next to the d64 kernel at the
same token count and width, and one full-depth encoder forward per 224 px image for each tower (random weights, warm).
Device-event timing; each shape is also checked against fp32 SDPA (max abs error / output range)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch, torch.nn.functional as F
from instantir_amd import ops
from instantir_amd.encoders import HipCLIPVision
dev = torch.device("cuda:0")
g = torch.Generator().manual_seed(0)
rnd = lambda *s: torch.randn(*s, generator=g).half().to(dev)
REP = int(os.environ.get("REP", "50"))


def timed(fn, rep):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(rep):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / rep


# the tower's own call: q | k one fused buffer, tokens padded 257 -> 264, 257 keys
for name, B, D, width in [("ViT-H/14", 1, 80, 1280), ("ViT-H/14", 2, 80, 1280), ("bigG/14", 1, 104, 1664), ("bigG/14", 2, 104, 1664)]:
    T, Tp = 257, 264
    for hd in (D, 64):
        h = width // hd
        qk, v = rnd(B * Tp, 2 * width), rnd(B * Tp, width)
        vt = v.T.contiguous()
        o = torch.empty(B * Tp, width, dtype=torch.half, device=dev)
        call = lambda: ops.attention(qk[:, :width], o, [(qk[:, width:], Tp, vt, Tp, T)], B, h, Tp, scale=hd ** -0.5, head_dim=hd)
        call(); torch.cuda.synchronize()
        sp = lambda x: x.float().reshape(B, Tp, h, hd)[:, :T].transpose(1, 2)
        ref = F.scaled_dot_product_attention(sp(qk[:, :width]), sp(qk[:, width:]), sp(v)).transpose(1, 2).reshape(B, T, width)
        err = ((o.float().reshape(B, Tp, width)[:, :T] - ref).abs().max() / ref.abs().max()).item()
        us = timed(call, REP)
        fl = 4.0 * B * h * Tp * hd * T
        print(f"attention {name:9s} B={B} heads={h:2d} d={hd:3d} T={T}: {us:7.1f} us  {fl / us / 1e6:6.1f} TFLOP/s  rel.err {err:.2e}",
              flush=True)


def tower_sd(D, inter, depth, proj):
    s = lambda *shape, sc=0.02: torch.randn(*shape, generator=g).mul_(sc).half().to(dev)
    sd = {"embeddings.patch_embedding.weight": s(D, 3, 14, 14), "embeddings.position_embedding.weight": s(257, D),
          "embeddings.class_embedding": s(D), "pre_layrnorm.weight": s(D, sc=0) + 1, "pre_layrnorm.bias": s(D),
          "post_layernorm.weight": s(D, sc=0) + 1, "post_layernorm.bias": s(D), "visual_projection.weight": s(proj, D)}
    for i in range(depth):
        p = f"encoder.layers.{i}."
        for n in ("layer_norm1", "layer_norm2"):
            sd[p + n + ".weight"], sd[p + n + ".bias"] = s(D, sc=0) + 1, s(D)
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            sd[p + "self_attn." + n + ".weight"], sd[p + "self_attn." + n + ".bias"] = s(D, D), s(D)
        sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"] = s(inter, D), s(inter)
        sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"] = s(D, inter), s(D)
    return sd


for name, D, inter, depth, proj in [("ViT-H/14", 1280, 5120, 32, 1024), ("bigG/14", 1664, 8192, 48, 1280)]:
    enc = HipCLIPVision(tower_sd(D, inter, depth, proj), dev, patch_size=14, num_heads=16, hidden_act="gelu")
    x = torch.randn(1, 3, 224, 224, generator=g).to(dev)
    ms = timed(lambda: enc(x, with_embeds=True), 10) / 1e3
    print(f"encoder {name:9s} {depth} layers, 1 image 224 px (hidden_states[-2] + image_embeds): {ms:6.2f} ms", flush=True)
    del enc
    torch.cuda.empty_cache()
