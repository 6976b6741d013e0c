"""GPU: the `--use_clip_encoder` branch (module/ip_adapter/utils.py:106-118) with a head-dim-80 CLIP tower (ViT-H/14's head
dim at the tiny geometry: 320 wide, 4 heads, GELU, 224 px) end to end: through `load_adapter_to_pipe` from a directory,
through `InstantIRPipeline.from_modules` from a transformers module, and through the CLI."""
import json
import math

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

BAR = 50.0


def psnr(got, want):
    mse = ((got - want) ** 2).mean().item()
    return 10 * math.log10(want.abs().max().item() ** 2 / max(mse, 1e-30))


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import dataclasses
    from safetensors.torch import save_file
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    from instantir_amd import lib, weights as W
    from instantir_amd.config import UNetConfig
    lib.load()
    cfg0 = UNetConfig.tiny()
    cfg = dataclasses.replace(cfg0, text_len=77, resampler=dataclasses.replace(cfg0.resampler, embedding_dim=320, seq_len=257))
    torch.manual_seed(31)
    vcfg = CLIPVisionConfig(hidden_size=320, intermediate_size=1280, num_hidden_layers=2, num_attention_heads=4, image_size=224,
                            patch_size=14, projection_dim=128, hidden_act="gelu", layer_norm_eps=1e-5)
    tower = CLIPVisionModelWithProjection(vcfg).eval()
    with torch.no_grad():
        for n, p in tower.named_parameters():
            if p.ndim == 1 and "norm" in n:
                p.add_(0.05 * torch.randn_like(p))
            elif "position_embedding" in n or "class_embedding" in n:
                p.copy_(0.3 * torch.randn_like(p))
            elif "q_proj.weight" in n or "k_proj.weight" in n:
                p.mul_(4.0)
    tsd = {k: v.half().float().contiguous() for k, v in tower.state_dict().items()}
    tower.load_state_dict(tsd)
    tdir = tmp_path_factory.mktemp("clip_h")
    save_file(tsd, str(tdir / "model.safetensors"))
    json.dump(vcfg.to_dict(), open(tdir / "config.json", "w"))
    full = W.synth_state_dict(W.unet_specs(cfg), 11)
    return dict(cfg=cfg, tower=tower, tsd=tsd, tdir=str(tdir), full=full, sda=W.synth_state_dict(W.aggregator_specs(cfg), 12),
                lora=W.synth_state_dict(W.lora_specs(cfg), 13))


def _adapter(cfg, full):
    """adapter.pt's dict layout (image_proj + ip_adapter) from the synthetic UNet tensors."""
    from instantir_amd import loaders
    ip = {}
    for idx, p in enumerate(loaders.attn_processor_paths(cfg)):
        if p.endswith("attn2"):
            for n in ("to_k_ip.weight", "to_v_ip.weight", "ln_k_ip.linear.weight", "ln_k_ip.linear.bias", "ln_v_ip.linear.weight",
                      "ln_v_ip.linear.bias"):
                ip[f"{idx}.{n}"] = full[f"{p}.processor.{n}"]
    pre = "encoder_hid_proj.image_projection_layers.0."
    return {"image_proj": {k[len(pre):]: v for k, v in full.items() if k.startswith(pre)}, "ip_adapter": ip}


def _pil(seed):
    return Image.fromarray(np.random.default_rng(seed).integers(0, 255, (96, 120, 3), dtype=np.uint8))


def test_load_adapter_with_clip_tower_directory(env):
    """(a) `load_adapter_to_pipe(..., use_clip_encoder=True)` + `pipe(ip_adapter_image=PIL)` gives the latents of the same pipe fed
    `ip_adapter_image_embeds` that transformers computed from the same tower (hidden_states[-2] of the image and the zero image)."""
    from instantir_amd import loaders
    from instantir_amd.encoders import HipCLIPVision, clip_preprocess
    from instantir_amd.pipeline import InstantIRPipeline
    from instantir_amd.schedulers import DDIMScheduler, LCMSingleStepScheduler
    cfg = env["cfg"]
    pipe = InstantIRPipeline(cfg, env["full"], scheduler=DDIMScheduler())
    loaders.load_adapter_to_pipe(pipe, _adapter(cfg, env["full"]), env["tdir"], use_clip_encoder=True, adapter_tokens=cfg.num_ip_tokens)
    assert isinstance(pipe.image_encoder, HipCLIPVision) and pipe.image_encoder.heads == 4 and pipe.image_encoder.head_dim == 80
    pipe.aggregator.load_state_dict(env["sda"])
    pipe.prepare_previewers(env["lora"], lora_alpha=16)
    g = torch.Generator().manual_seed(5)
    B, H = 1, 16
    kw = dict(image=torch.randn(B, 4, H, H, generator=g) * 0.8,
              prompt_embeds=torch.randn(B, cfg.text_len, cfg.cross_attention_dim, generator=g).half().float(),
              pooled_prompt_embeds=torch.randn(B, cfg.pooled_dim, generator=g).half().float(),
              negative_prompt_embeds=torch.randn(B, cfg.text_len, cfg.cross_attention_dim, generator=g).half().float(),
              negative_pooled_prompt_embeds=torch.randn(B, cfg.pooled_dim, generator=g).half().float(),
              init_noise=torch.randn(B, 4, H, H, generator=g), output_type="latent", num_inference_steps=3, guidance_scale=5.0,
              previewer_scheduler=LCMSingleStepScheduler.from_config(pipe.scheduler.config))
    pil = _pil(1)
    got = pipe(ip_adapter_image=[pil], **kw).images.float().cpu()
    px = clip_preprocess([pil])
    with torch.no_grad():
        f = env["tower"](pixel_values=px, output_hidden_states=True).hidden_states[-2]
        z = env["tower"](pixel_values=torch.zeros_like(px), output_hidden_states=True).hidden_states[-2]
    want = pipe(ip_adapter_image_embeds=[torch.stack([z, f])], **kw).images.float().cpu()
    assert torch.isfinite(got).all()
    assert psnr(got, want) >= BAR


def test_from_modules_takes_the_tower_config(env):
    """(b) `from_modules(image_encoder=<transformers module>)` reads heads / activation / eps from the module's config (a ViT-H
    tower is 16 heads of 80, not D // 64 heads of 64) and encodes exactly as the directory path does."""
    from instantir_amd import loaders
    from instantir_amd.encoders import HipCLIPVision, clip_preprocess
    from instantir_amd.pipeline import InstantIRPipeline
    from instantir_amd.schedulers import DDIMScheduler
    cfg = env["cfg"]
    pipe = InstantIRPipeline.from_modules(unet=dict(env["full"]), aggregator=env["sda"], scheduler=DDIMScheduler(), unet_config=cfg,
                                          image_encoder=env["tower"])
    enc = pipe.image_encoder
    assert isinstance(enc, HipCLIPVision) and enc.heads == 4 and enc.head_dim == 80 and enc.act == HipCLIPVision(
        env["tsd"], "cuda:0", num_heads=4, hidden_act="gelu").act
    ref = InstantIRPipeline(cfg, env["full"], scheduler=DDIMScheduler())
    loaders.load_adapter_to_pipe(ref, _adapter(cfg, env["full"]), env["tdir"], use_clip_encoder=True, adapter_tokens=cfg.num_ip_tokens)
    px = clip_preprocess([_pil(2), _pil(3)])
    f, z = enc.encode_image_pair(px)
    fr, zr = ref.image_encoder.encode_image_pair(px)
    assert torch.equal(f, fr) and torch.equal(z, zr)
    with torch.no_grad():
        want = env["tower"](pixel_values=px, output_hidden_states=True).hidden_states[-2]
    assert psnr(f.float().cpu(), want) >= 45


def test_infer_cli_with_clip_encoder(env, tmp_path):
    """(c) `python -m instantir_amd.infer --use_clip_encoder --vision_encoder_path <tower dir>` over a checkpoint tree writes the
    image a twin pipeline assembled from the same tensors writes, bit for bit."""
    from test_infer_cli_gpu import _write_checkpoint_tree
    from transformers import CLIPTokenizer
    import instantir_amd.infer as cli
    from instantir_amd.config import VAEConfig
    from instantir_amd.encoders import HipCLIPText, HipCLIPVision
    from instantir_amd.pipeline import InstantIRPipeline
    from instantir_amd.schedulers import DDPMScheduler, LCMSingleStepScheduler
    from instantir_amd.vae import HipVAE
    cfg, vc = env["cfg"], VAEConfig.tiny()
    mem = _write_checkpoint_tree(tmp_path, cfg, vc)
    src, out = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    Image.fromarray(np.random.default_rng(4).integers(0, 255, (128, 128, 3), dtype=np.uint8)).save(src / "x.png")
    args = cli.build_parser().parse_args([
        "--sdxl_path", str(tmp_path / "sdxl"), "--instantir_path", str(tmp_path / "instantir"), "--vision_encoder_path", env["tdir"],
        "--use_clip_encoder", "--test_path", str(src), "--out_path", str(out), "--num_inference_steps", "2", "--width", "128",
        "--height", "128", "--cfg", "5.0", "--seed", "7", "--adapter_tokens", str(cfg.num_ip_tokens)])
    orig = cli.resize_img
    cli.resize_img = lambda im, **kw: orig(im, max_side=128, min_side=128, **kw)
    try:
        torch.manual_seed(123)
        cli.main(args, torch.device("cuda:0"))
    finally:
        cli.resize_img = orig
    got = np.asarray(Image.open(out / "x.png"))

    dev = "cuda:0"
    tok = CLIPTokenizer.from_pretrained(str(tmp_path / "sdxl" / "tokenizer"))
    mk = lambda texts: tok(texts, padding="max_length", max_length=tok.model_max_length, truncation=True, return_tensors="pt").input_ids
    pipe = InstantIRPipeline(cfg, mem["full"], scheduler=DDPMScheduler(), vae=HipVAE(vc, mem["vae"], dev), device=dev,
                             image_encoder=HipCLIPVision(env["tsd"], dev, num_heads=4, hidden_act="gelu"),
                             text_encoder=HipCLIPText(mem["tes"][0][0], dev, hidden_act="quick_gelu"),
                             text_encoder_2=HipCLIPText(mem["tes"][1][0], dev, hidden_act="gelu"), tokenizer=mk, tokenizer_2=mk)
    pipe.prepare_previewers(mem["lora"], lora_alpha=mem["alpha"])
    pipe.aggregator.load_state_dict(mem["agg"])
    lq, _ = orig(Image.open(src / "x.png").convert("RGB"), max_side=128, min_side=128, width=128, height=128)
    g = torch.Generator(device=dev).manual_seed(7)
    torch.manual_seed(123)
    img = pipe(image=[lq], prompt=[cli.DEFAULT_PROMPT], negative_prompt=[cli.DEFAULT_NEG_PROMPT], ip_adapter_image=[lq],
               num_inference_steps=2, generator=g, guidance_scale=5.0, previewer_scheduler=LCMSingleStepScheduler.from_config(pipe.scheduler.config),
               preview_start=args.preview_start, control_guidance_end=args.creative_start).images[0]
    want = np.asarray(img.resize([128, 128], Image.BILINEAR))
    assert got.shape == want.shape and np.array_equal(got, want)
