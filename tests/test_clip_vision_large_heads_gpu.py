"""GPU: `HipCLIPVision` at the two CLIP towers SDXL IP-Adapter users load with `--use_clip_encoder`
(module/ip_adapter/utils.py:106-118) -- OpenCLIP ViT-H/14 (head dim 80) and ViT-bigG/14 (head dim 104) at their real widths
and 224 px, a few layers deep -- against transformers' CLIPVisionModelWithProjection with the same random weights."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu


def psnr(got, want):
    mse = ((got - want) ** 2).mean().item()
    return 10 * math.log10(want.abs().max().item() ** 2 / max(mse, 1e-30))


def _tower(hidden, inter, proj, layers, seed):
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    torch.manual_seed(seed)
    c = CLIPVisionConfig(hidden_size=hidden, intermediate_size=inter, num_hidden_layers=layers, num_attention_heads=16,
                         image_size=224, patch_size=14, projection_dim=proj, hidden_act="gelu", layer_norm_eps=1e-5)
    m = CLIPVisionModelWithProjection(c).eval()
    with torch.no_grad():
        for n, p in m.named_parameters():
            if p.ndim == 1 and "norm" in n:
                p.add_(0.05 * torch.randn_like(p))
            elif "position_embedding" in n or "class_embedding" in n:
                p.copy_(0.3 * torch.randn_like(p))
            elif "q_proj.weight" in n or "k_proj.weight" in n:
                p.mul_(4.0)                 # scores well away from uniform, so the softmax is exercised
    sd = {k: v.half().float() for k, v in m.state_dict().items()}
    m.load_state_dict(sd)
    return m, sd


@pytest.mark.parametrize("name,hidden,inter,proj,layers", [("ViT-H/14", 1280, 5120, 1024, 3), ("ViT-bigG/14", 1664, 8192, 1280, 2)])
def test_large_head_towers_match_transformers(name, hidden, inter, proj, layers):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from instantir_amd.encoders import HipCLIPVision
    m, sd = _tower(hidden, inter, proj, layers, seed=hidden)
    x = torch.randn(2, 3, 224, 224, generator=torch.Generator().manual_seed(hidden + 1))
    with torch.no_grad():
        out = m(pixel_values=x, output_hidden_states=True)
        outz = m(pixel_values=torch.zeros(1, 3, 224, 224), output_hidden_states=True)
    enc = HipCLIPVision(sd, "cuda:0", num_heads=16, hidden_act="gelu", eps=1e-5)
    assert enc.head_dim == hidden // 16
    h, emb = enc(x, with_embeds=True)
    assert h.shape == (2, 257, hidden) and emb.shape == (2, proj)
    assert psnr(h.float().cpu(), out.hidden_states[-2]) >= 45, name
    assert psnr(emb.float().cpu(), out.image_embeds) >= 40, name
    f, z = enc.encode_image_pair(x)
    assert psnr(f.float().cpu(), out.hidden_states[-2]) >= 45, name
    assert psnr(z.float().cpu(), outz.hidden_states[-2].expand(2, -1, -1)) >= 45, name
    _, ez = enc(torch.zeros(1, 3, 224, 224), with_embeds=True)
    assert psnr(ez.float().cpu(), outz.image_embeds) >= 40, name


def test_other_head_dims_are_refused():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from instantir_amd.encoders import HipCLIPVision
    for D, heads in ((384, 4), (1280, 10), (1280, 13)):          # head dims 96, 128, and 1280 / 13 (not a whole number)
        with pytest.raises(ValueError, match=r"\(64, 80, 104\)"):
            HipCLIPVision({"vision_model.embeddings.patch_embedding.weight": torch.zeros(D, 3, 14, 14)}, "cuda:0", num_heads=heads)
