"""VAE flash attention (`iir_attention_1h`, `HipVAE.enable_flash_attention()`) beside the default path, on one MI355X.

  kernel:  attention_1h at D = 512, bf16, one image, T = 16384 against the launches it replaces on the same inputs (fp32 score
           GEMM + row softmax + P.V GEMM; the V^T projection runs in both paths and is timed on its own), alternating pairs;
           the kernel alone at T = 24576 and 65536.
  vae:     SDXL-shaped VAE, synthetic bf16 weights: decode and moments at 1024^2 switch off / on (alternating), decode at
           1536 x 1024 untiled with the switch against `enable_tiling()`, and the arena bytes of each.
Times are device events around REP back-to-back calls after a warm-up; each line gives the median of ROUNDS such windows and
their spread.  `python tools/vae_flash_bench.py [kernel] [vae]`."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from instantir_amd import ops

dev = torch.device("cuda:0")
REP = int(os.environ.get("REP", "5"))
ROUNDS = int(os.environ.get("ROUNDS", "5"))
DT = torch.bfloat16


def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REP):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REP


def compare(named):
    """Alternating windows of every candidate; prints median and min..max in ms, returns the medians."""
    for _, fn in named:
        fn()
    torch.cuda.synchronize()
    t = {n: [] for n, _ in named}
    for _ in range(ROUNDS):
        for n, fn in named:
            t[n].append(window(fn))
    med = {}
    for n, _ in named:
        v = sorted(t[n])
        med[n] = v[len(v) // 2]
        print(f"    {n:44s} {med[n]:9.3f} ms   ({v[0]:.3f} .. {v[-1]:.3f})", flush=True)
    return med


def kernel_leg():
    g = torch.Generator().manual_seed(0)
    rnd = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(DT).to(dev)
    D = 512
    for T in (16384, 24576, 65536):
        q, k, vt, b = rnd(T, D), rnd(T, D), rnd(D, T), rnd(D)
        o = torch.empty(T, D, dtype=DT, device=dev)
        flops = 4.0 * T * T * D
        print(f"attention D={D} bf16 one image T={T}  ({flops / 1e12:.2f} TFLOP)")
        cands = [("attention_1h", lambda: ops.attention_1h(q, o, k, vt, T, 1, T, T, D ** -0.5, bias=b))]
        if T <= 16384:
            s32 = torch.empty(T, T, dtype=torch.float32, device=dev)
            pr = torch.empty(T, T, dtype=DT, device=dev)
            o2 = torch.empty(T, D, dtype=DT, device=dev)
            n, wv = rnd(T, D), rnd(D, D, scale=D ** -0.5)
            vt2 = torch.empty(D, T, dtype=DT, device=dev)

            def old():
                ops.gemm(q, k, s32, out_scale=D ** -0.5)
                ops.softmax_rows_f32(s32, pr)
                ops.gemm(pr, vt, o2, bias=b)
            cands += [("score GEMM + softmax + P.V GEMM (default path)", old),
                      ("  score GEMM alone", lambda: ops.gemm(q, k, s32, out_scale=D ** -0.5)),
                      ("  softmax alone", lambda: ops.softmax_rows_f32(s32, pr)),
                      ("  P.V GEMM alone", lambda: ops.gemm(pr, vt, o2, bias=b)),
                      ("V^T projection (both paths)", lambda: ops.gemm(wv, n, vt2))]
        med = compare(cands)
        print(f"    attention_1h: {flops / med['attention_1h'] / 1e9:.0f} TFLOP/s", flush=True)


def vae_leg():
    from instantir_amd import weights as W
    from instantir_amd.config import VAEConfig
    from instantir_amd.vae import HipVAE
    vc = VAEConfig.sdxl()
    hv = HipVAE(vc, W.synth_state_dict(W.vae_decoder_specs(vc) + W.vae_encoder_specs(vc), 31, device=dev, dtype=DT), dev)
    g = torch.Generator().manual_seed(1)

    def arena_of(fn, flash, tiling=False):
        """bytes the arena needs for this call alone (a fresh sizing run)"""
        hv.enable_flash_attention(flash)
        hv.enable_tiling(tiling)
        hv._sized = {}
        fn()
        torch.cuda.synchronize()
        return max(hv._sized.values()) * 2

    def setup(flash, tiling=False):
        hv.enable_flash_attention(flash)
        hv.enable_tiling(tiling)

    z = torch.randn(1, 4, 128, 128, generator=g).to(dev) * vc.scaling_factor
    img = (torch.rand(1, 3, 1024, 1024, generator=g) * 2 - 1).to(dev)
    print("SDXL VAE bf16, 1024^2, one image")
    for name, fn in (("decode_latent", lambda: hv.decode_latent(z, "pt")), ("moments", lambda: hv.moments(img))):
        a_off, a_on = arena_of(fn, False), arena_of(fn, True)
        print(f"  {name}: arena {a_off / 2 ** 20:.0f} MiB (switch off) / {a_on / 2 ** 20:.0f} MiB (switch on)")
        compare([(f"{name} switch off", lambda: (setup(False), fn())), (f"{name} switch on", lambda: (setup(True), fn()))])
    z2 = torch.randn(1, 4, 192, 128, generator=g).to(dev) * vc.scaling_factor
    fn = lambda: hv.decode_latent(z2, "pt")
    a_t, a_f = arena_of(fn, False, True), arena_of(fn, True, False)
    print(f"SDXL VAE bf16, 1536 x 1024 decode: arena {a_t / 2 ** 20:.0f} MiB (tiled, switch off) / {a_f / 2 ** 20:.0f} MiB (untiled, switch on)")
    compare([("decode_latent enable_tiling()", lambda: (setup(False, True), fn())),
             ("decode_latent enable_tiling() + switch", lambda: (setup(True, True), fn())),
             ("decode_latent untiled, switch on", lambda: (setup(True, False), fn()))])
    setup(False)


if __name__ == "__main__":
    legs = sys.argv[1:] or ["kernel", "vae"]
    print(torch.cuda.get_device_name(0), f"REP={REP} ROUNDS={ROUNDS}")
    if "kernel" in legs:
        kernel_leg()
    if "vae" in legs:
        vae_leg()
