"""GPU: NIQE's device statistics (ops.niqe_stats / iir_niqe_stats) against the fp64 restatement of the contract and the fp32
restatement of the kernel's own arithmetic (tests/niqe_ref.py), their determinism, and the `instantir_amd.niqe`, `metrics.niqe`
and CLI wiring.

Bounds (DESIGN.md section 7 "NIQE"; none is taken from what the kernel gives):
  b, the element error bound of m, and b_sigma, that of sigma: the worst case over the rounding points is far above 3e-4 (a window
      whose variance cancels), so, as for LPIPS, b = 3 x the largest gap of the fp32 CPU restatement to fp64 over this file's
      inputs, computed on the CPU before anything is launched (about 1.5e-5; the value is printed and recorded in
      profiles/niqe_test_figures.log).
  sums of squares, of |v| and of sigma: |kernel - fp64| <= niqe_ref.sum_bounds(b, b_sigma), and |kernel - fp32 restatement| <=
      4 x 2^-24 of the figure (what is left there is the order of the fp64 additions).
  counts: |kernel - fp64| <= the number of the block-and-map's reference elements with |v| <= b_v (b for v0, 2 b max|m| for a
      product); the test first asserts of its own inputs that this number is at most 1 % of the block's elements.  Against the
      fp32 restatement the counts are equal.
  features: every alpha within one table step of the one from fp64 sums; the score within 3 x the CPU rounding model's gap.
Every operand lies inside a larger buffer (NaN around fp32, 255 around uint8, content at most 250), and every stored pixel outside
the block-grid part -- the cropped border and the ragged remainder -- is wild: NaN in an fp32 source (the contract says such a
pixel is never read), 255 in a uint8 one.  The figures must be those of the part alone, bit for bit."""
import json
import math

import numpy as np
import pytest
import torch

import niqe_ref as R

pytestmark = pytest.mark.gpu

ULPS = 4 * 2.0 ** -24
PAD = 4096
COUNTS = [5 * q + k for q in range(5) for k in (0, 1)]
SUMS = [c for c in range(26) if c not in COUNTS]
_shape_id = lambda sc: "x".join(map(str, sc[0])) + f"-crop{sc[1]}"


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from instantir_amd import lib
    lib.load()
    return torch.device("cuda:0")


def _guarded(x, dev):
    """`x` on the device as a view into a larger buffer: NaN around fp32, 255 around uint8."""
    t = torch.from_numpy(x)
    if x.dtype == np.uint8:
        buf = torch.full((t.numel() + 2 * PAD,), 255, dtype=torch.uint8, device=dev)
    else:
        buf = torch.full((t.numel() + 2 * PAD,), float("nan"), device=dev)
    view = buf[PAD:PAD + t.numel()].view(t.shape)
    view.copy_(t)
    return view, buf


def _part(u8, c):
    """The block-grid part of uint8 (N, H, W, C) on its own."""
    nbh, nbw = R.grid(u8.shape[1], u8.shape[2], c)
    return np.ascontiguousarray(u8[:, c:c + 96 * nbh, c:c + 96 * nbw])


def _wild(u8, c, form):
    """The stored image in the asked form with every pixel outside the block-grid part made wild."""
    nbh, nbw = R.grid(u8.shape[1], u8.shape[2], c)
    inside = np.zeros(u8.shape[1:3], bool)
    inside[c:c + 96 * nbh, c:c + 96 * nbw] = True
    if form == "u8":
        assert u8.max() <= 250
        return np.where(inside[None, :, :, None], u8, np.uint8(255))
    return np.where(inside[None, None], R.as_f32(u8), np.float32("nan"))


_REF = {}


def _reference(si):
    """Computed once per shape: the picture, fp64 and fp32-restatement sums, the element bounds and what follows from them."""
    if si not in _REF:
        shape, c = R.GPU_SHAPES[si]
        u8 = R.picture(20 + si, *shape)
        gm, gs = R.element_gaps(u8, c)
        b, bs = 3 * gm, 3 * gs
        bounds, flips = R.sum_bounds(u8, c, b, bs)
        _REF[si] = dict(u8=u8, s64=R.stats(u8, c), s32=R.stats32(u8, c), b=b, bs=bs, bounds=bounds, flips=flips)
    return _REF[si]


_MODEL = []


def _model():
    """A synthetic pristine model: the fp64 restatement's fit to two seeded pictures of 30 blocks each (a full-rank covariance)."""
    if not _MODEL:
        _MODEL.append(R.fit([R.stats(R.picture(s, 1, 1, 480, 576)) for s in (31, 32)]))
    return _MODEL[0]


# ---- the kernel against the restatements ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["u8", "f32"])
@pytest.mark.parametrize("si", range(len(R.GPU_SHAPES)), ids=[_shape_id(s) for s in R.GPU_SHAPES])
def test_sums_and_counts_match_both_restatements(dev, si, form):
    from instantir_amd import ops
    shape, c = R.GPU_SHAPES[si]
    ref = _reference(si)
    n_elems = np.array([96 * 96, 48 * 48], dtype=np.float64).reshape(1, 2, 1, 1)
    share = (ref["flips"] / n_elems).max()
    print(f"niqe {_shape_id(R.GPU_SHAPES[si])} {form} b {ref['b']:.3e} b_sigma {ref['bs']:.3e} largest share of |v| <= b_v {share:.4%}")
    assert ref["b"] <= 3e-4 and share <= 0.01                                   # the condition under which the count test means something
    src, buf = _guarded(_wild(ref["u8"], c, form), dev)
    got = ops.niqe_stats(src, crop_border=c)
    torch.cuda.synchronize()
    nbh, nbw = R.grid(shape[2], shape[3], c)
    assert got.dtype == torch.float64 and got.shape == (shape[0], 2, nbh * nbw, 26) and got.device == src.device
    got = got.cpu().numpy()
    assert np.isfinite(got).all()
    s64, s32 = ref["s64"], ref["s32"]
    dc = np.abs(got[..., COUNTS] - s64[..., COUNTS]).reshape(got.shape[:3] + (5, 2))
    err = np.abs(got[..., SUMS] - s64[..., SUMS]) / ref["bounds"][..., SUMS]
    rel32 = np.abs(got[..., SUMS] - s32[..., SUMS]) / np.abs(s32[..., SUMS])
    print(f"niqe {_shape_id(R.GPU_SHAPES[si])} {form} sums: worst |kernel - fp64| / bound {err.max():.3e}, worst |kernel - fp32 restatement| "
          f"/ figure {rel32.max():.3e}; counts: largest difference to fp64 {dc.max():.0f} (allowed up to {ref['flips'].max():.0f}), to the "
          f"fp32 restatement {np.abs(got[..., COUNTS] - s32[..., COUNTS]).max():.0f}")
    assert (got[..., COUNTS] == np.round(got[..., COUNTS])).all()
    assert (dc <= ref["flips"][..., None]).all()
    assert (err <= 1.0).all(), err.max()
    assert np.array_equal(got[..., COUNTS], s32[..., COUNTS])
    assert (rel32 <= ULPS).all(), rel32.max()
    # every count pair leaves out the exact zeros only, and the two sides' squares are both there
    assert (got[..., COUNTS].reshape(got.shape[:3] + (5, 2)).sum(-1) <= n_elems).all() and (got[..., SUMS] > 0).all()
    assert bool((buf[:PAD] == 255).all() if form == "u8" else torch.isnan(buf[:PAD]).all())


@pytest.mark.parametrize("si", range(len(R.GPU_SHAPES)), ids=[_shape_id(s) for s in R.GPU_SHAPES])
def test_only_the_block_grid_part_counts_and_both_forms_give_equal_bits(dev, si):
    from instantir_amd import ops
    shape, c = R.GPU_SHAPES[si]
    u8 = _reference(si)["u8"]
    alone = ops.niqe_stats(_guarded(_part(u8, c), dev)[0])
    for form in ("u8", "f32"):
        assert torch.equal(ops.niqe_stats(_guarded(_wild(u8, c, form), dev)[0], crop_border=c), alone), form
    ws = torch.empty(R.BLOCK * R.BLOCK * 64, dtype=torch.float64, device=dev)                    # a caller's workspace, larger than needed
    assert torch.equal(ops.niqe_stats(_guarded(_wild(u8, c, "u8"), dev)[0], crop_border=c, ws=ws), alone)
    with pytest.raises(ValueError, match="ws needs"):
        ops.niqe_stats(_guarded(_part(u8, c), dev)[0], ws=ws[:16])


def test_two_launches_and_batching_are_bit_equal(dev):
    from instantir_amd import ops
    u8 = _reference(1)["u8"]
    src = torch.from_numpy(u8).to(dev)
    a, b = ops.niqe_stats(src), ops.niqe_stats(src)
    assert torch.equal(a, b)
    for n in range(2):
        assert torch.equal(ops.niqe_stats(src[n:n + 1].contiguous()), a[n:n + 1])
    f32 = torch.from_numpy(R.as_f32(u8)).to(dev)
    assert torch.equal(ops.niqe_stats(f32), a) and torch.equal(ops.niqe_stats(f32[1:].contiguous()), a[1:])


# ---- features, score, fit ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("si", range(len(R.GPU_SHAPES)), ids=[_shape_id(s) for s in R.GPU_SHAPES])
def test_features_and_score_from_device_sums(dev, si):
    from instantir_amd import metrics as M, niqe as NQ
    shape, c = R.GPU_SHAPES[si]
    ref = _reference(si)
    mu, cov = _model()
    model = NQ.NIQE(mu, cov)
    f64, f32 = R.features(ref["s64"]), R.features(ref["s32"])
    want, want32 = R.score((mu, cov), ref["s64"]), R.score((mu, cov), ref["s32"])
    gap = np.abs(want32 - want)
    src = _guarded(_wild(ref["u8"], c, "u8"), dev)[0]
    from instantir_amd import ops
    feats = NQ.features(ops.niqe_stats(src, crop_border=c))
    got = model(src, crop_border=c)
    assert got.dtype == np.float64 and np.array_equal(got, model.score_features(feats))
    da = np.abs(feats - f64)[..., R.ALPHA_COLUMNS].max()
    print(f"niqe {_shape_id(R.GPU_SHAPES[si])} score {got} fp64 {want} |kernel - fp64| {np.abs(got - want)} CPU rounding model's gap {gap}; "
          f"largest alpha difference {da:.4f} (fp32 restatement {np.abs(f32 - f64)[..., R.ALPHA_COLUMNS].max():.4f})")
    assert np.isfinite(feats).all() and da <= 0.001 + 1e-12
    assert np.isfinite(want).all() and (want > 0).all() and (np.abs(got - want) <= 3 * gap).all()
    listed = M.niqe(src, model, crop_border=c)
    assert listed == got.tolist() if shape[0] > 1 else listed == got[0]


def test_fit_on_the_device_equals_the_restatements_model(dev):
    from instantir_amd import niqe as NQ
    pics = [R.picture(41, 1, 1, 288, 384), R.picture(42, 1, 3, 300, 200, flat_rows=101)]
    s64, s32 = [R.stats(p) for p in pics], [R.stats32(p) for p in pics]
    keep = lambda sl: [tuple(s[0, 0, :, 25] > 0.75 * s[0, 0, :, 25].max()) for s in sl]
    assert keep(s64) == keep(s32) and sum(map(sum, keep(s64))) >= 12 and not all(keep(s64)[1])    # the rule drops the flat blocks
    (mu, cov), (mu32, cov32) = R.fit(s64), R.fit(s32)
    model = NQ.NIQE.fit([torch.from_numpy(pics[0]).to(dev), pics[1][0]], device=dev)
    other = [c for c in range(36) if c not in R.ALPHA_COLUMNS]
    gap_mu, gap_cov = np.abs(mu32 - mu)[other].max(), np.abs(cov32 - cov).max()
    print(f"niqe fit: mu alpha columns {np.abs(model.mu - mu)[R.ALPHA_COLUMNS].max():.2e}, other columns {np.abs(model.mu - mu)[other].max():.3e} "
          f"(CPU gap {gap_mu:.3e}), cov {np.abs(model.cov - cov).max():.3e} (CPU gap {gap_cov:.3e})")
    assert np.abs(model.mu - mu)[R.ALPHA_COLUMNS].max() <= 0.001 + 1e-12
    assert np.abs(model.mu - mu)[other].max() <= 3 * gap_mu and np.abs(model.cov - cov).max() <= 3 * gap_cov


def test_refusals_on_the_device(dev):
    from instantir_amd import niqe as NQ, ops
    with pytest.raises(ValueError, match="at least two"):
        ops.niqe_stats(torch.zeros(1, 1, 191, 191, device=dev))
    model = NQ.NIQE(np.zeros(36), np.eye(36))
    with pytest.raises(ValueError, match="at least two"):
        model(torch.zeros(3, 100, 400, device=dev), crop_border=3)
    flat = model(torch.full((1, 96, 192), 0.5, device=dev))
    assert flat.shape == (1,) and math.isnan(flat[0])                              # a constant image: no finite block


# ---- the CLI ----------------------------------------------------------------------------------------------------------------------
def test_cli_niqe(tmp_path, dev):
    from PIL import Image
    import instantir_amd.infer as cli
    from instantir_amd import metrics as M, niqe as NQ
    src = tmp_path / "in"
    src.mkdir()
    Image.fromarray(R.picture(51, 1, 3, 128, 256)[0]).save(src / "a.png")
    params = tmp_path / "pris.npz"
    NQ.NIQE(*_model()).save(str(params))
    common = ["--synthetic", "tiny", "--num_inference_steps", "2", "--batch_size", "1", "--cfg", "5.0", "--test_path", str(src),
              "--width", "256", "--height", "128"]
    runs = {"plain": ["--input_fidelity", "--metrics_crop", "2"],
            "both": ["--input_fidelity", "--metrics_crop", "2", "--niqe_path", str(params)],
            "alone": ["--niqe_path", str(params)]}
    orig = cli.resize_img
    cli.resize_img = lambda im, **kw: orig(im, max_side=256, min_side=128, **kw)      # keep the tiny nets tiny
    try:
        for name, flags in runs.items():
            torch.manual_seed(123)          # the VAE posterior sample draws from the global RNG
            cli.main(cli.build_parser().parse_args(common + flags + ["--out_path", str(tmp_path / name)]), dev)
    finally:
        cli.resize_img = orig
    saved = Image.open(tmp_path / "both" / "a.png").convert("RGB")
    assert saved.size == (256, 128)
    assert (tmp_path / "plain" / "a.png").read_bytes() == (tmp_path / "both" / "a.png").read_bytes() == (tmp_path / "alone" / "a.png").read_bytes()
    plain, both, alone = (json.load(open(tmp_path / n / "metrics.json")) for n in ("plain", "both", "alone"))
    model = NQ.NIQE.from_file(str(params))
    assert set(plain["files"]["a.png"]) == {"input_psnr", "input_ssim"} and "niqe" not in plain["settings"]
    assert set(both["files"]["a.png"]) == {"input_psnr", "input_ssim", "niqe", "input_niqe"}
    assert both["settings"]["niqe"] == {"path": str(params), "crop_border": 2, "input": True}
    # without the flag nothing of the report changes: the scored run's report minus the NIQE entries is the plain run's, byte for byte
    strip = lambda rep: {"settings": {k: v for k, v in rep["settings"].items() if k != "niqe"},
                         "files": {f: {k: v for k, v in row.items() if "niqe" not in k} for f, row in rep["files"].items()},
                         "mean": {k: v for k, v in rep["mean"].items() if "niqe" not in k}}
    assert json.dumps(strip(both), indent=1, sort_keys=True) == open(tmp_path / "plain" / "metrics.json").read()
    twin, twin_in = M.niqe(saved, model, crop_border=2, device=dev), M.niqe(Image.open(src / "a.png").convert("RGB"), model, crop_border=2, device=dev)
    assert math.isfinite(twin) and math.isfinite(twin_in) and twin > 0 and twin_in > 0
    assert both["files"]["a.png"]["niqe"] == twin == both["mean"]["niqe"] and both["files"]["a.png"]["input_niqe"] == twin_in == both["mean"]["input_niqe"]
    assert alone["settings"] == {"niqe": {"path": str(params), "crop_border": 0, "input": False}}
    assert alone["files"] == {"a.png": {"niqe": M.niqe(saved, model, device=dev)}} and set(alone["mean"]) == {"niqe"}


def _write_checkpoint_tree(root, cfg, vc):
    """A tiny SDXL + InstantIR + DINOv2 checkpoint tree in the on-disk formats infer.py reads, from
    seeded synthetic tensors: the equivalent of the one tests/test_infer_cli_gpu.py builds, kept here so that neither file
    imports the other."""
    import json
    from safetensors.torch import save_file
    from tokenizers import pre_tokenizers
    from transformers import CLIPTextConfig, CLIPTextModelWithProjection, CLIPTokenizer, Dinov2Config, Dinov2Model
    from instantir_amd import loaders, weights as W
    sdxl, iir, dino_dir = root / "sdxl", root / "instantir", root / "dino"
    for d in ("unet", "vae", "text_encoder", "text_encoder_2", "tokenizer", "tokenizer_2", "scheduler"):
        (sdxl / d).mkdir(parents=True)
    iir.mkdir(); dino_dir.mkdir()
    c = lambda sd: {k: v.contiguous() for k, v in sd.items()}
    # -- SDXL UNet: base weights only; the TA-IP processors / Resampler travel in adapter.pt
    full = W.synth_state_dict(W.unet_specs(cfg), 11)
    base = {k: v for k, v in full.items() if ".processor." not in k and not k.startswith("encoder_hid_proj.")}
    save_file(c(base), str(sdxl / "unet" / "diffusion_pytorch_model.fp16.safetensors"))
    json.dump({"block_out_channels": list(cfg.block_out_channels), "down_block_types": ["DownBlock2D", "CrossAttnDownBlock2D", "CrossAttnDownBlock2D"],
               "transformer_layers_per_block": [1, cfg.transformer_depth[1], cfg.transformer_depth[2]], "layers_per_block": cfg.layers_per_block,
               "attention_head_dim": [ch // 64 for ch in cfg.block_out_channels], "cross_attention_dim": cfg.cross_attention_dim,
               "addition_embed_type": "text_time", "addition_time_embed_dim": cfg.addition_time_embed_dim,
               "projection_class_embeddings_input_dim": cfg.add_embed_in, "norm_num_groups": cfg.norm_groups, "in_channels": 4,
               "out_channels": 4}, open(sdxl / "unet" / "config.json", "w"))
    vae_sd = W.synth_state_dict(W.vae_decoder_specs(vc) + W.vae_encoder_specs(vc), 14)
    save_file(c(vae_sd), str(sdxl / "vae" / "diffusion_pytorch_model.safetensors"))
    json.dump({"block_out_channels": list(vc.block_out_channels), "layers_per_block": vc.layers_per_block, "latent_channels": 4,
               "in_channels": 3, "norm_num_groups": vc.norm_groups, "scaling_factor": vc.scaling_factor}, open(sdxl / "vae" / "config.json", "w"))
    # -- tokenizers: byte-level vocabulary without merges (every character is a token); <|endoftext|> has the largest id
    chars = sorted(set(pre_tokenizers.ByteLevel.alphabet()))
    vocab = {ch: i for i, ch in enumerate(chars)}
    vocab.update({ch + "</w>": len(chars) + i for i, ch in enumerate(chars)})
    vocab["<|startoftext|>"] = len(vocab)
    vocab["<|endoftext|>"] = len(vocab)
    for t in ("tokenizer", "tokenizer_2"):
        CLIPTokenizer(vocab=vocab, merges=[], model_max_length=cfg.text_len).save_pretrained(str(sdxl / t))
    # -- text encoders (width 64 each -> 128-wide context = cfg.cross_attention_dim; projection = pooled_dim)
    torch.manual_seed(5)
    tes = []
    for sub, act in (("text_encoder", "quick_gelu"), ("text_encoder_2", "gelu")):
        tc = CLIPTextConfig(vocab_size=len(vocab), hidden_size=64, intermediate_size=256, num_hidden_layers=2, num_attention_heads=1,
                            max_position_embeddings=cfg.text_len, projection_dim=cfg.pooled_dim, hidden_act=act, eos_token_id=2,
                            bos_token_id=vocab["<|startoftext|>"], pad_token_id=1)
        sd = {k: v.half().float().contiguous() for k, v in CLIPTextModelWithProjection(tc).state_dict().items()}
        save_file(sd, str(sdxl / sub / "model.safetensors"))
        json.dump({"hidden_act": act, "eos_token_id": 2, "layer_norm_eps": 1e-5}, open(sdxl / sub / "config.json", "w"))
        tes.append((sd, act))
    json.dump({"num_train_timesteps": 1000, "beta_start": 0.00085, "beta_end": 0.012, "beta_schedule": "scaled_linear", "steps_offset": 1,
               "timestep_spacing": "leading", "prediction_type": "epsilon", "_class_name": "EulerDiscreteScheduler"},
              open(sdxl / "scheduler" / "scheduler_config.json", "w"))
    # -- DINOv2 directory
    torch.manual_seed(8)
    dm = Dinov2Model(Dinov2Config(hidden_size=cfg.resampler.embedding_dim, num_hidden_layers=2, num_attention_heads=1, patch_size=14,
                                  image_size=224, mlp_ratio=4))
    dino_sd = {k: v.half().float().contiguous() for k, v in dm.state_dict().items()}
    save_file(dino_sd, str(dino_dir / "model.safetensors"))
    json.dump({"patch_size": 14, "num_attention_heads": 1, "layer_norm_eps": 1e-6}, open(dino_dir / "config.json", "w"))
    # -- InstantIR files: adapter.pt (dict layout), aggregator.pt, previewer LoRA in diffusers naming with a network alpha
    paths = loaders.attn_processor_paths(cfg)
    ip = {}
    for idx, p in enumerate(paths):
        if p.endswith("attn2"):
            for n in ("to_k_ip.weight", "to_v_ip.weight", "ln_k_ip.linear.weight", "ln_k_ip.linear.bias", "ln_v_ip.linear.weight",
                      "ln_v_ip.linear.bias"):
                ip[f"{idx}.{n}"] = full[f"{p}.processor.{n}"]
    pre = "encoder_hid_proj.image_projection_layers.0."
    torch.save({"image_proj": {k[len(pre):]: v for k, v in full.items() if k.startswith(pre)}, "ip_adapter": ip}, str(iir / "adapter.pt"))
    agg = W.synth_state_dict(W.aggregator_specs(cfg), 12)
    torch.save(agg, str(iir / "aggregator.pt"))
    lora = W.synth_state_dict(W.lora_specs(cfg), 13)
    f = {}
    for k, v in lora.items():
        k = k.replace(".lora_A.weight", ".lora.down.weight").replace(".lora_B.weight", ".lora.up.weight").replace(".processor.", ".")
        f["unet." + k] = v
    f["unet.down_blocks.0.resnets.0.conv1.alpha"] = torch.tensor(4.0)
    torch.save(f, str(iir / "previewer_lora_weights.bin"))


def test_cli_niqe_from_checkpoint_files(tmp_path, dev):
    """`--niqe_path` with `--input_fidelity` through the file-loading path of the CLI (a fabricated checkpoint tree, string
    prompts): `niqe` per file and on average, `input_niqe` beside it, both equal to `metrics.niqe` on the saved / input file."""
    import dataclasses
    from PIL import Image
    import instantir_amd.infer as cli
    from instantir_amd import metrics as M, niqe as NQ
    from instantir_amd.config import UNetConfig, VAEConfig
    cfg0 = UNetConfig.tiny()
    cfg = dataclasses.replace(cfg0, text_len=77, resampler=dataclasses.replace(cfg0.resampler, seq_len=257))
    _write_checkpoint_tree(tmp_path, cfg, VAEConfig.tiny())
    src, out = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    Image.fromarray(R.picture(52, 1, 3, 128, 256)[0]).save(src / "x.png")
    params = tmp_path / "pris.npz"
    NQ.NIQE(*_model()).save(str(params))
    args = cli.build_parser().parse_args([
        "--sdxl_path", str(tmp_path / "sdxl"), "--instantir_path", str(tmp_path / "instantir"), "--vision_encoder_path", str(tmp_path / "dino"),
        "--test_path", str(src), "--out_path", str(out), "--num_inference_steps", "2", "--width", "256", "--height", "128", "--cfg", "5.0",
        "--seed", "7", "--adapter_tokens", str(cfg.num_ip_tokens), "--niqe_path", str(params), "--input_fidelity"])
    orig = cli.resize_img
    cli.resize_img = lambda im, **kw: orig(im, max_side=256, min_side=128, **kw)
    try:
        torch.manual_seed(123)
        cli.main(args, dev)
    finally:
        cli.resize_img = orig
    rep = json.load(open(out / "metrics.json"))
    model = NQ.NIQE.from_file(str(params))
    row = rep["files"]["x.png"]
    assert set(row) == {"input_psnr", "input_ssim", "niqe", "input_niqe"} and rep["settings"]["niqe"]["input"] is True
    assert row["niqe"] == M.niqe(Image.open(out / "x.png").convert("RGB"), model, device=dev) == rep["mean"]["niqe"]
    assert row["input_niqe"] == M.niqe(Image.open(src / "x.png").convert("RGB"), model, device=dev) == rep["mean"]["input_niqe"]
    assert math.isfinite(row["niqe"]) and math.isfinite(row["input_niqe"])
