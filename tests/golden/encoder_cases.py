"""The encoder towers and calls that make_encoder_bits.py (GPU, output bits) and make_encoder_trace.py (CPU, launch trace)
both replay: `HipDinov2`, `HipCLIPVision` and `HipCLIPText` through their public surface only (constructor, call,
`encode_image_pair`), with state dicts synthesised under the Hugging Face parameter names -- no `transformers`.  Each tower
reads its depth from the keys.  The smallest towers that reach every branch of instantir_amd/encoders.py:

* DINOv2, D = 128 in 2 heads, 2 layers, stored table of a 4 x 4 grid, B = 2: 56 px (T = 17 -> 24 rows, the native table),
  84 px (T = 37 -> 40 rows, the bicubic table; left out where `native_only`), and `encode_image_pair` at 56 px.
* CLIP vision, 2 layers, 56 px, patch 14, B = 2: head dims 64, 80 and 104 as (D, heads) = (128, 2), (320, 4), (832, 8) -- the
  GEMMs take K in whole 64-wide tiles, so D is the smallest common multiple of the head dim and 64; at 64 quick-GELU and GELU;
  at 64 and 80 with and without `with_embeds` (which runs one more layer); `encode_image_pair` at 64.
* CLIP text, D = 128, 3 layers, vocabulary 100, B = 2, T = 77 -> 80 rows, one sequence ending early: (hidden_act,
  eos_token_id) = (quick_gelu, 2) and (gelu, 98), `clip_skip` None and 1, with and without `text_projection.weight`.

`draw(rng, shape, kind)` supplies the values: kind "w" a matrix, "b" a bias, "g" a norm gain, "ls" a LayerScale vector, "e" an
embedding / position table, "x" pixel values.
"""
import numpy as np
import torch

PATCH, GRID, PROJ, VOCAB, TEXT_LEN = 14, 4, 96, 100, 77


def draw_normal(rng, shape, kind):
    """fp16-representable random normals; norms perturbed around (1, 0), LayerScale in [0.5, 1]."""
    if kind == "ls":
        v = rng.uniform(0.5, 1.0, shape)
    else:
        v = rng.standard_normal(shape) * {"w": float(np.prod(shape[1:])) ** -0.5, "b": 0.1, "g": 0.05, "e": 0.3, "x": 1.0}[kind]
        if kind == "g":
            v = 1.0 + v
    return torch.from_numpy(v.astype(np.float32)).half().float()


def draw_ints(rng, shape, kind):
    """Small integers, |v| <= 4 (LayerScale 1 or 2): every sum and product of the weight packing is exact in fp32."""
    v = rng.randint(1, 3, shape) if kind == "ls" else rng.randint(-4, 5, shape)
    return torch.from_numpy(v.astype(np.float32))


def _synth(spec, rng, draw):
    return {name: draw(rng, shape, kind) for name, shape, kind in spec}


def _linear(name, n, k):
    return [(name + ".weight", (n, k), "w"), (name + ".bias", (n,), "b")]


def _norm(name, D):
    return [(name + ".weight", (D,), "g"), (name + ".bias", (D,), "b")]


def dino_spec(D, depth):
    s = [("embeddings.patch_embeddings.projection.weight", (D, 3, PATCH, PATCH), "w"),
         ("embeddings.patch_embeddings.projection.bias", (D,), "b"),
         ("embeddings.cls_token", (1, 1, D), "e"), ("embeddings.position_embeddings", (1, 1 + GRID * GRID, D), "e")]
    for i in range(depth):
        p = f"encoder.layer.{i}"
        s += _norm(p + ".norm1", D) + _norm(p + ".norm2", D)
        for n in ("attention.query", "attention.key", "attention.value", "output.dense"):
            s += _linear(f"{p}.attention.{n}", D, D)
        s += _linear(p + ".mlp.fc1", 4 * D, D) + _linear(p + ".mlp.fc2", D, 4 * D)
        s += [(p + ".layer_scale1.lambda1", (D,), "ls"), (p + ".layer_scale2.lambda1", (D,), "ls")]
    return s + _norm("layernorm", D)


def _clip_layers(prefix, D, depth):
    s = []
    for i in range(depth):
        p = f"{prefix}encoder.layers.{i}"
        s += _norm(p + ".layer_norm1", D) + _norm(p + ".layer_norm2", D)
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            s += _linear(f"{p}.self_attn.{n}", D, D)
        s += _linear(p + ".mlp.fc1", 4 * D, D) + _linear(p + ".mlp.fc2", D, 4 * D)
    return s


def clip_vision_spec(D, depth, proj=True):
    v = "vision_model."
    s = [(v + "embeddings.patch_embedding.weight", (D, 3, PATCH, PATCH), "w"), (v + "embeddings.class_embedding", (D,), "e"),
         (v + "embeddings.position_embedding.weight", (1 + GRID * GRID, D), "e")]
    s += _norm(v + "pre_layrnorm", D) + _clip_layers(v, D, depth) + _norm(v + "post_layernorm", D)
    return s + ([("visual_projection.weight", (PROJ, D), "w")] if proj else [])


def clip_text_spec(D, depth, proj):
    t = "text_model."
    s = [(t + "embeddings.token_embedding.weight", (VOCAB, D), "e"), (t + "embeddings.position_embedding.weight", (TEXT_LEN, D), "e")]
    s += _clip_layers(t, D, depth) + _norm(t + "final_layer_norm", D)
    return s + ([("text_projection.weight", (PROJ, D), "w")] if proj else [])


def text_ids(rng, eos):
    """Two sequences of 77 ids; the first ends early (eot = the highest id for the legacy eos_token_id 2, else the first eos)."""
    ids = rng.randint(3, 97, (2, TEXT_LEN))
    ids[0, 20:] = eos if eos != 2 else 99
    ids[1, 76] = eos if eos != 2 else 99
    return torch.from_numpy(ids.astype(np.int64))


def cases(draw, device, native_only=False):
    """Yields (key, call); `call()` returns {name: tensor or None} -- what the public surface returned.  Towers are built
    while iterating, before the call of their first case; construction launches nothing."""
    from instantir_amd.encoders import HipCLIPText, HipCLIPVision, HipDinov2
    px = GRID * PATCH

    rng = np.random.RandomState(20261018)
    dino = HipDinov2(_synth(dino_spec(128, 2), rng, draw), device)
    x = draw(rng, (2, 3, px, px), "x")
    yield "dino.56", lambda x=x: {"out": dino(x)}
    if not native_only:
        x84 = draw(rng, (2, 3, 6 * PATCH, 6 * PATCH), "x")
        yield "dino.84", lambda x=x84: {"out": dino(x)}
    yield "dino.pair56", lambda x=x: dict(zip(("feats", "zero"), dino.encode_image_pair(x)))

    for D, heads, acts, embeds in ((128, 2, ("quick_gelu", "gelu"), (False, True)), (320, 4, ("quick_gelu",), (False, True)),
                                   (832, 8, ("quick_gelu",), (False,))):
        rng = np.random.RandomState(20261018 + D)
        sd = _synth(clip_vision_spec(D, 2), rng, draw)
        x = draw(rng, (2, 3, px, px), "x")
        for act in acts:
            enc = HipCLIPVision(sd, device, num_heads=heads, hidden_act=act)
            for emb in embeds:
                if emb:
                    yield f"clipv.hd{D // heads}.{act}.embeds", lambda enc=enc, x=x: dict(zip(("hidden", "embeds"), enc(x, with_embeds=True)))
                else:
                    yield f"clipv.hd{D // heads}.{act}", lambda enc=enc, x=x: {"hidden": enc(x)}
            if D == 128 and act == "quick_gelu":
                yield "clipv.hd64.pair", lambda enc=enc, x=x: dict(zip(("feats", "zero"), enc.encode_image_pair(x)))

    for act, eos in (("quick_gelu", 2), ("gelu", 98)):
        for proj in (False, True):
            rng = np.random.RandomState(20261018 + eos)               # the projected tower = the plain one + text_projection
            enc = HipCLIPText(_synth(clip_text_spec(128, 3, proj), rng, draw), device, hidden_act=act, eos_token_id=eos)
            ids = text_ids(np.random.RandomState(eos), eos)
            for skip in (None, 1):
                yield (f"clipt.{act}.eos{eos}.{'proj' if proj else 'noproj'}.skip{skip or 0}",
                       lambda enc=enc, ids=ids, skip=skip: dict(zip(("hidden", "pooled"), enc(ids, clip_skip=skip))))
