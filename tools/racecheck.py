"""Race screen: every kernel here is deterministic, so repeated launches on the same inputs must be BIT-identical; any
difference (or a mismatch against the fp32 reference) is reported with its location.  GEMM tiles x epilogues,
transposed column range, conv, attention."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch, torch.nn.functional as F
from instantir_amd import ops
from instantir_amd.packing import pair_rows, conv_weight_nhwc
dev = torch.device("cuda:0")
REP = int(os.environ.get("REP", "30"))
g = torch.Generator().manual_seed(1)
rnd = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).half()
bad_total = 0
ONLY = os.environ.get("ONLY")          # run only the cases whose name contains this substring (the unnamed blocks below always run)

def screen(name, launch, want, outs_shape, rtol=4e-3, atol=4e-3):
    global bad_total
    if ONLY and ONLY not in name:
        return
    first = None; nd = 0; where = None
    for it in range(REP):
        outs = [torch.zeros(s, dtype=torch.half, device=dev) for s in outs_shape]
        launch(*outs)
        torch.cuda.synchronize()
        cat = torch.cat([o.flatten() for o in outs])
        if first is None:
            first = cat
            err = (cat.float().cpu() - want).abs()
            ok = bool((err <= atol + rtol * want.abs()).all())
        elif not torch.equal(cat, first):
            nd += 1
            idx = (cat != first).nonzero().flatten()
            where = (int(idx.numel()), idx[:4].tolist())
    bad_total += (not ok) + nd
    print(f"{name:56s} ref_ok={ok} nondeterministic_runs={nd}/{REP - 1} {where or ''}", flush=True)

for (M, N, K) in [(2048, 1280, 1280), (1000, 640, 1280), (2048, 1280, 5120)]:
    x, w, b, res = rnd(M, K), rnd(N, K, scale=K ** -0.5), rnd(N), rnd(M, N)
    xd, wd, bd, rd = x.to(dev), w.to(dev), b.to(dev), res.to(dev)
    want = (x.float() @ w.float().T + b.float() + res.float()).flatten()
    for tile in (0, 1, 2, 3, 4, 5, 35):
        screen(f"gemm {M}x{N}x{K} tile {tile} bias+res", lambda o: ops.gemm(xd, wd, o, bias=bd, res=rd, tile=tile), want, [(M, N)])
    h = x.float() @ w.float().T + b.float()
    wantg = (h[:, :N // 2] * F.gelu(h[:, N // 2:])).flatten()
    wp, bp = pair_rows(w[:N // 2], w[N // 2:]).to(dev), pair_rows(b[:N // 2], b[N // 2:]).to(dev)
    for tile in (0, 2, 3, 4, 5):
        screen(f"gemm {M}x{N}x{K} tile {tile} GEGLU", lambda o: ops.gemm(xd, wp, o, bias=bp, epi=ops.EPI_GEGLU, tile=tile), wantg, [(M, N // 2)])
M, C, K = 2048, 640, 640
x, w = rnd(M, K), rnd(3 * C, K, scale=K ** -0.5)
full = x.float() @ w.float().T
xd, wd = x.to(dev), w.to(dev)
for tile in (0, 2, 3, 5):
    screen(f"gemm q|k|v {M}x{3*C}x{K} tile {tile} (V transposed)", lambda qk, vt: ops.gemm(xd, wd, qk, out_t=(vt, 2 * C), tile=tile),
           torch.cat([full[:, :2 * C].flatten(), full[:, 2 * C:].T.flatten()]), [(M, 2 * C), (C, M)])
R, H, Cin, Cout = 2, 32, 1280, 1280
x, w, b = rnd(R, Cin, H, H), rnd(Cout, Cin, 3, 3, scale=(9 * Cin) ** -0.5), rnd(Cout)
want = F.conv2d(x.float(), w.float(), b.float(), padding=1).permute(0, 2, 3, 1).reshape(-1, Cout).flatten()
xd, wd, bd = x.permute(0, 2, 3, 1).contiguous().to(dev), conv_weight_nhwc(w).to(dev), b.to(dev)
for tile in (0, 2, 5, 35):
    screen(f"conv3x3 {R}x{H}x{H} {Cin}->{Cout} tile {tile}", lambda o: ops.conv2d(xd, wd, o, bias=bd, tile=tile), want, [(R * H * H, Cout)])
B, heads, T = 2, 20, 1024
Cc = heads * 64
qkv = rnd(B * T, 2 * Cc).to(dev); vt = rnd(Cc, B * T).to(dev)
q4 = qkv[:, :Cc].float().reshape(B, T, heads, 64).transpose(1, 2); k4 = qkv[:, Cc:].float().reshape(B, T, heads, 64).transpose(1, 2)
v4 = vt.float().T.reshape(B, T, heads, 64).transpose(1, 2)
want = F.scaled_dot_product_attention(q4, k4, v4).transpose(1, 2).reshape(B * T, Cc).flatten().cpu()
screen(f"attention B={B} h={heads} T={T}", lambda o: ops.attention(qkv[:, :Cc], o, [(qkv[:, Cc:], T, vt, T, T)], B, heads, T), want, [(B * T, Cc)])
# adaptive projected guidance: iir_apg_project + iir_sched_step with IIR_STEP_APG (fp32 planes; prev against plain CFG at the identity parameters
# eta = 1, r = 0, beta = 0, which equal it algebraically), bit-identical over REP launches at the library defaults
for apB in (1, 8):
    ap_x = (torch.randn(apB, 4, 128, 128, generator=g) * 0.8).to(dev)
    ap_eps = rnd(2 * apB * 128 * 128, 64).to(dev)
    ap_a0 = torch.randn(apB, 4, 128, 128, generator=g).to(dev)
    ap_coef = torch.tensor([7.0, 0.9, 0.3, 0.8, 0.5, 0.0, 0.0, 0.0], device=dev)
    ap_ref, ap_ws = torch.empty_like(ap_x), ops.apg_workspace(apB, dev)
    ops.sched_step(ap_eps, apB, ap_coef, ap_x, ap_ref)
    for ap_name, ap_par in (("identity", [1.0, 0.0, 0.0, 0.0]), ("defaults", [0.0, 15.0, -0.5, 0.0])):
        ap_pd = torch.tensor(ap_par, device=dev)
        first = None; nd = 0
        for it in range(REP):
            a, sa, o = ap_a0.clone(), torch.zeros(2 * apB, device=dev), torch.zeros_like(ap_x)
            ops.apg_project(ap_eps, apB, ap_coef, ap_x, (a, sa, ap_pd), ap_ws)
            ops.sched_step(ap_eps, apB, ap_coef, ap_x, o, apg=(a, sa, ap_pd))
            torch.cuda.synchronize()
            cat = torch.cat([o.flatten(), a.flatten(), sa])
            if first is None: first = cat
            elif not torch.equal(cat, first): nd += 1
        ok = ap_name != "identity" or bool(((first[:ap_x.numel()] - ap_ref.flatten()).abs() <= 1e-4 + 1e-5 * ap_ref.flatten().abs()).all())
        bad_total += (not ok) + nd
        print(f"{'apg_project + sched_step_apg B=%d %s' % (apB, ap_name):56s} ref_ok={ok} nondeterministic_runs={nd}/{REP - 1}", flush=True)
# LQ fidelity guidance: iir_lq_fidelity_f32 at 128^2 latents (x0', prev in place and the history plane; against torch's conv form of
# the interior, where no tap is dropped), radius 0 (the one-thread-per-element launch), 5 and 24 (the tile launch)
from instantir_amd import lq_fidelity as lqf
lf_x0, lf_z, lf_p0 = (torch.randn(1, 4, 128, 128, generator=g).to(dev) for _ in range(3))
lf_wc = torch.tensor([0.75, 0.625], device=dev)
for lf_sigma in (0.0, 1.5, 8.0):
    lf_t = lqf.taps(lf_sigma)
    lf_taps = torch.tensor(lf_t, dtype=torch.float64).float().to(dev) if lf_t else None
    lf_r = lqf.radius(lf_sigma)
    lf_d = lf_z - lf_x0
    if lf_r:
        k2 = torch.outer(lf_taps, lf_taps)[None, None].repeat(4, 1, 1, 1)
        lf_d = F.pad(F.conv2d(lf_d, k2, groups=4), [lf_r] * 4)
    lf_want = lf_x0 + 0.75 * lf_d
    first = None; nd = 0
    for it in range(REP):
        p, o, hs = lf_p0.clone(), torch.zeros_like(lf_x0), torch.zeros_like(lf_x0)
        ops.lq_fidelity(lf_x0, lf_z, lf_wc, p, o, taps=lf_taps, hist=hs)
        torch.cuda.synchronize()
        cat = torch.cat([o.flatten(), p.flatten(), hs.flatten()])
        if first is None: first = cat
        elif not torch.equal(cat, first): nd += 1
    inner = (slice(None), slice(None), slice(lf_r, 128 - lf_r), slice(lf_r, 128 - lf_r))
    ok = bool(((first[:lf_x0.numel()].view_as(lf_x0)[inner] - lf_want[inner]).abs() <= 1e-4).all())
    bad_total += (not ok) + nd
    print(f"{'lq_fidelity 1x4x128x128 sigma %g (radius %d)' % (lf_sigma, lf_r):56s} ref_ok={ok} nondeterministic_runs={nd}/{REP - 1}", flush=True)
# device resampling (ops.resample): float mode against torch's antialiased interpolate (bilinear, bicubic; the same definition),
# quantised mode against the same interpolate one axis at a time with floor(v + 0.5) clamped to [0, 255] after each (the clip
# between the passes is part of the mode), both source layouts; bit-identical over REP launches
def rs_ref(x, out, f, q):
    if not q:
        return F.interpolate(x, size=out, mode=f, antialias=True, align_corners=False)
    for size in ((x.shape[2], out[1]), out):
        x = (F.interpolate(x, size=size, mode=f, antialias=True, align_corners=False) + 0.5).floor().clamp(0, 255)
    return x
for (rs_in, rs_out, rs_f) in [((384, 512), (768, 1024), "bilinear"), ((1024, 1024), (256, 256), "bicubic"), ((1024, 1024), (2048, 2048), "lanczos"),
                              ((257, 131), (129, 67), "bicubic")]:
    rs_u8 = torch.randint(0, 256, (1, rs_in[0], rs_in[1], 3), generator=g, dtype=torch.uint8).to(dev)
    rs_f32 = rs_u8.permute(0, 3, 1, 2).float().contiguous()
    for rs_src, rs_name in ((rs_u8, "uint8"), (rs_f32, "fp32")):
        for rs_q in (False, True):
            first = None; nd = 0
            for it in range(REP):
                o = ops.resample(rs_src, rs_out, rs_f, quantize=rs_q)
                torch.cuda.synchronize()
                if first is None: first = o
                elif not torch.equal(o, first): nd += 1
            # quantised: a sample on a rounding boundary may flip in either pass, and a flipped intermediate moves the second sum by < 1
            ok = rs_f == "lanczos" or bool(((first - rs_ref(rs_f32, rs_out, rs_f, rs_q)).abs() <= (2.0 if rs_q else 1e-2)).all())
            bad_total += (not ok) + nd
            print(f"{'resample %s %dx%d->%dx%d %s%s' % (rs_f, *rs_in, *rs_out, rs_name, ' quantised' if rs_q else ''):56s} ref_ok={ok} "
                  f"nondeterministic_runs={nd}/{REP - 1}", flush=True)
print("TOTAL anomalies:", bad_total)
sys.exit(1 if bad_total else 0)
