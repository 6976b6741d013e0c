"""CPU: the two hooks of the oracle loops (oracle.pipeline.denoise, loop_ref.sigma_denoise) and the hooks of tests/loop_ref.py.
Three steps with preview_start = 0.34 and control_guidance_end = 0.67: an Aggregator-only step, a previewed step and a step
without the Aggregator.  Every comparison is on bits."""
import pytest
import torch

import apg_ref
import loop_ref as lr
from loop_ref import pag_oracle_attn  # noqa: F401  (fixture)

KW = dict(preview_start=0.34, control_guidance_end=0.67)
G = 5.0


@pytest.fixture(scope="module")
def env():
    return lr.tiny_env()


def passthrough(P, cfg, xin, t, ctx, text_embeds, tid, ip_main, down, mid):
    from oracle import nets
    return nets.unet_forward(P, cfg, xin, t, ctx, text_embeds, tid, ip_main, down, mid)


def cfg_line(rows, i, t, x, coef):
    u, c = rows
    return u + G * (c - u)


def identity(rows, i, t, x, coef):
    c, = rows
    return c


@pytest.mark.parametrize("loop,g,guide", [("ddim", G, cfg_line), ("ddim", 1.0, identity), ("dpm", G, cfg_line)],
                         ids=["ddim-cfg", "ddim-nocfg", "dpm-karras"])
def test_hooks_that_restate_the_loop_give_its_bits(env, loop, g, guide):
    if loop == "ddim":
        run = lambda **kw: lr.denoise(env, g, num_inference_steps=3, **KW, **kw)
        variants = [{}, dict(guidance_rescale=0.7)] if g > 1 else [{}]
    else:
        run = lambda **kw: lr.sigma_denoise(env, "dpm", 3, guidance_scale=g, karras=True, **KW, **kw)
        variants = [{}]                                                   # (the sigma loop has no guidance_rescale)
    for kw in variants:
        plain = run(**kw)
        assert torch.isfinite(plain).all()
        assert torch.equal(run(main_unet=passthrough, guide=guide, **kw), plain), kw


@pytest.mark.parametrize("g,groups", [(G, 3), (1.0, 2)])
def test_guide_receives_the_row_groups_of_the_main_unet_hook(env, pag_oracle_attn, g, groups):
    from instantir_amd import pag
    B = env[4]["B"]
    seen = []

    def guide(rows, i, t, x, coef):
        seen.append((i, [tuple(r.shape) for r in rows], tuple(x.shape), len(coef)))
        return lr.perturbed(g, 3.0)(rows, i, t, x, coef)
    paths = pag.select("mid", pag.attn1_paths(env[0]))
    out = lr.denoise(env, g, main_unet=lr.pag_unet(paths, B), guide=guide, num_inference_steps=2, **KW)
    assert torch.isfinite(out).all() and out.shape == env[4]["lq"].shape
    assert seen == [(i, [(B, 4, 16, 16)] * groups, (B, 4, 16, 16), 2) for i in range(2)]


def test_apg_hook_starts_each_call_afresh(env, monkeypatch):
    """The momentum argument is 0 at step 0 alone, step 0 is handed no average, and a second call of the SAME hook object gives the
    first call's bits (a leaked average would move step 0's projection)."""
    par = (0.0, 6.0, -0.5)
    calls = []
    orig = apg_ref.apg_eps

    def apg_eps(u, c, x, a_prev, coef, eta, r, beta, fp32=False):
        calls.append((a_prev is None, beta))
        return orig(u, c, x, a_prev, coef, eta, r, beta, fp32=fp32)
    monkeypatch.setattr(apg_ref, "apg_eps", apg_eps)
    hook = lr.apg(G, par)
    a = lr.denoise(env, G, guide=hook, num_inference_steps=3, **KW)
    b = lr.denoise(env, G, guide=hook, num_inference_steps=3, **KW)
    assert calls == [(True, 0.0), (False, -0.5), (False, -0.5)] * 2
    assert torch.equal(a, b)
    assert not torch.equal(a, lr.denoise(env, G, num_inference_steps=3, **KW))
