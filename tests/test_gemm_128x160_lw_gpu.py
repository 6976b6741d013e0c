"""The 128x160 loader-wave tile (id 54: one workgroup per CU, 4 compute + 4 loader waves, 3-deep ring) against the tiles it stands
in for -- 25 (two 64x160 workgroups per CU, the round-3 choice for these shapes) and 24 (the 4-wave 128x160 tile).  The K
accumulation order of an output element does not depend on the tile, so every output must be bit-identical: plain, bias +
residual, row bias (temb), LayerNorm and GroupNorm partials, convs with per-image row remaps into a concat buffer.  Plus a race
screen of the new build beside a busy second stream, in the form of tests/test_concurrency_gpu.py."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILES = (54, 0, 25, 24)          # 0: the automatic choice, which must be 54 on these shapes
GEMMS = [(4096, 1280, 1280), (4096, 1280, 5120), (8192, 640, 2560)]
CONVS = [(2, 64, 64, 640, 640), (2, 64, 64, 320, 640), (2, 64, 32, 1280, 1280)]     # (R, H, W, Cin, Cout), 3x3


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from instantir_amd import lib
    lib.load()
    return torch.device("cuda:0")


def _rand(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).half()


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.half else torch.int32)


def _same(results, what):
    """results: one tuple of tensors per entry of TILES; all must equal the first bit for bit"""
    for tile, res in zip(TILES[1:], results[1:]):
        for k, (a, b) in enumerate(zip(results[0], res)):
            assert torch.equal(_bits(a), _bits(b)), f"{what}: tile {tile} output {k} differs from tile {TILES[0]} " \
                                                    f"({int((_bits(a) != _bits(b)).sum())} elements)"


def test_automatic_choice_is_the_new_tile():
    from instantir_amd import ops
    for M, N, K in GEMMS:
        assert ops.gn_supported(M, N, K) and ops.ln_parts(M, N, K) == N // 160
    for R, H, W, Cin, Cout in CONVS:
        assert ops.gn_supported(R * H * W, Cout, 9 * Cin, True)


@pytest.mark.parametrize("M,N,K", GEMMS)
@pytest.mark.parametrize("kind", ["plain", "bias_res", "rowbias", "gn"])
def test_gemm_bit_identical_across_tiles(dev, M, N, K, kind):
    from instantir_amd import ops
    g = torch.Generator().manual_seed(M + N + K)
    a, w = _rand(g, M, K).to(dev), _rand(g, N, K, scale=K ** -0.5).to(dev)
    bias, res, rb = _rand(g, N).to(dev), _rand(g, M, N).to(dev), _rand(g, 2, N).to(dev)
    results = []
    for tile in TILES:
        out = torch.zeros(M, N, dtype=torch.half, device=dev)
        if kind == "plain":
            ops.gemm(a, w, out, tile=tile)
            results.append((out,))
        elif kind == "bias_res":
            ops.gemm(a, w, out, bias=bias, res=res, tile=tile)
            results.append((out,))
        elif kind == "rowbias":
            ops.gemm(a, w, out, bias=bias, rowbias=rb, rows_per_rb=M // 2, act=ops.ACT_SILU, tile=tile)
            results.append((out,))
        else:
            part = torch.zeros(M // 64, N, 2, dtype=torch.float32, device=dev)
            ops.gemm(a, w, out, bias=bias, res=res, gn_out=part, tile=tile)
            results.append((out, part))
    torch.cuda.synchronize()
    _same(results, f"gemm {M}x{N}x{K} {kind}")


def _ln_case(dev, M, N, K):
    """ln_stats_out needs tile = 0: the automatic launch of this process, with its stored output"""
    from instantir_amd import ops
    g = torch.Generator().manual_seed(M * 3 + K)
    a, w = _rand(g, M, K).to(dev), _rand(g, N, K, scale=K ** -0.5).to(dev)
    bias, res = _rand(g, N).to(dev), _rand(g, M, N).to(dev)
    out = torch.zeros(M, N, dtype=torch.half, device=dev)
    st = torch.zeros(ops.ln_parts(M, N, K), M, 2, dtype=torch.float32, device=dev)
    ops.gemm(a, w, out, bias=bias, res=res, ln_out=st)
    torch.cuda.synchronize()
    return out.cpu(), st.cpu()


@pytest.mark.parametrize("M,N,K", GEMMS)
def test_gemm_ln_partials_match_the_round3_tile(dev, M, N, K, tmp_path):
    """automatic launch here (tile 54) against the automatic launch of a child process with IIR_T4_LW=0 (tile 25): the switch
    is read once per process"""
    got = _ln_case(dev, M, N, K)
    dst = tmp_path / "ln.pt"
    env = dict(os.environ, IIR_T4_LW="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "ln_child", str(M), str(N), str(K), str(dst)], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    want = torch.load(dst)
    for k, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(_bits(a), _bits(b)), f"ln_stats_out case {M}x{N}x{K}: output {k} differs from the IIR_T4_LW=0 launch"


@pytest.mark.parametrize("R,H,W,Cin,Cout", CONVS)
@pytest.mark.parametrize("kind", ["bias_rowbias", "remap_concat", "gn"])
def test_conv_bit_identical_across_tiles(dev, R, H, W, Cin, Cout, kind):
    from instantir_amd import ops
    from instantir_amd.packing import conv_weight_nhwc
    g = torch.Generator().manual_seed(H + W + Cin + Cout)
    HW = H * W
    x = _rand(g, R, H, W, Cin).to(dev)
    w = conv_weight_nhwc(_rand(g, Cout, Cin, 3, 3, scale=(9 * Cin) ** -0.5)).to(dev)
    bias, rb = _rand(g, Cout).to(dev), _rand(g, R, Cout).to(dev)
    results = []
    for tile in TILES:
        if kind == "bias_rowbias":
            out = torch.zeros(R * HW, Cout, dtype=torch.half, device=dev)
            ops.conv2d(x, w, out, bias=bias, rowbias=rb, rows_per_rb=HW, tile=tile)
            results.append((out,))
        elif kind == "remap_concat":
            # skip-concat write: image i's rows start at i * (HW + 64) of a buffer 320 columns wider than the output;
            # the residual's images sit (HW + 128) rows apart
            buf = torch.zeros(R * (HW + 64), Cout + 320, dtype=torch.half, device=dev)
            resb = _rand(torch.Generator().manual_seed(5), R * (HW + 128), Cout).to(dev)
            ops.conv2d(x, w, buf[:, :Cout], bias=bias, rowbias=rb, rows_per_rb=HW, res=resb, y_img_rows=HW + 64,
                       res_img_rows=HW + 128, tile=tile)
            results.append((buf,))
        else:
            out = torch.zeros(R * HW, Cout, dtype=torch.half, device=dev)
            part = torch.zeros(R * HW // 64, Cout, 2, dtype=torch.float32, device=dev)
            res = _rand(torch.Generator().manual_seed(6), R * HW, Cout).to(dev)
            ops.conv2d(x, w, out, bias=bias, rowbias=rb, rows_per_rb=HW, res=res, gn_out=part, tile=tile)
            results.append((out, part))
    torch.cuda.synchronize()
    if kind == "remap_concat":
        buf = results[0][0].view(R, HW + 64, Cout + 320)
        assert buf[:, HW:].abs().max().item() == 0 and buf[:, :, Cout:].abs().max().item() == 0, "written outside the image rows"
    _same(results, f"conv {R}x{H}x{W} {Cin}->{Cout} {kind}")


def test_new_tile_reproducible_beside_a_busy_stream(dev):
    from instantir_amd import ops
    from instantir_amd.packing import conv_weight_nhwc
    g = torch.Generator().manual_seed(4)
    rnd = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).half().to(dev)
    side = torch.cuda.Stream()
    nx, nw, no = rnd(4096, 1280), rnd(2560, 1280, scale=0.03), torch.empty(4096, 2560, dtype=torch.half, device=dev)
    nq, nvt, nao = rnd(2 * 2048, 2 * 640), rnd(640, 2 * 2048), torch.empty(2 * 2048, 640, dtype=torch.half, device=dev)
    ncx, ncw, nco = rnd(2, 32, 32, 1280), rnd(1280, 3, 3, 1280, scale=0.01), torch.empty(2 * 32 * 32, 1280, dtype=torch.half, device=dev)

    def noise():
        with torch.cuda.stream(side):
            for _ in range(3):
                ops.gemm(nx, nw, no)
                ops.attention(nq[:, :640], nao, [(nq[:, 640:], 2048, nvt, 2048, 2048)], 2, 10, 2048)
                ops.conv2d(ncx, ncw, nco)

    def screen(name, launch, shapes, dtypes):
        first = None
        for it in range(8):
            outs = [torch.zeros(s, dtype=d, device=dev) for s, d in zip(shapes, dtypes)]
            noise()
            launch(*outs)
            torch.cuda.synchronize()
            cat = torch.cat([_bits(o).flatten().long() for o in outs])
            if first is None:
                first = cat
            else:
                assert torch.equal(cat, first), f"{name}: launch {it} differs from launch 0 ({int((cat != first).sum())} elements)"

    M, N, K = 4096, 1280, 5120
    x, w, b, res = rnd(M, K), rnd(N, K, scale=K ** -0.5), rnd(N), rnd(M, N)
    h16, f32 = torch.half, torch.float32
    screen("gemm tile 54, bias + residual", lambda o: ops.gemm(x, w, o, bias=b, res=res, tile=54), [(M, N)], [h16])
    screen("gemm tile 54, gn_out", lambda o, p: ops.gemm(x, w, o, bias=b, res=res, gn_out=p, tile=54), [(M, N), (M // 64, N, 2)], [h16, f32])
    screen("gemm automatic, ln_out", lambda o, p: ops.gemm(x, w, o, res=res, ln_out=p), [(M, N), (N // 160, M, 2)], [h16, f32])
    cx, cw, cb = rnd(2, 64, 64, 640), conv_weight_nhwc(rnd(640, 640, 3, 3, scale=0.02)), rnd(640)
    screen("conv3x3 level 1, tile 54", lambda o: ops.conv2d(cx, cw, o, bias=cb, tile=54), [(2 * 64 * 64, 640)], [h16])
    screen("conv3x3 level 1, tile 54, gn_out", lambda o, p: ops.conv2d(cx, cw, o, bias=cb, gn_out=p, tile=54),
           [(2 * 64 * 64, 640), (2 * 64, 640, 2)], [h16, f32])


if __name__ == "__main__" and len(sys.argv) == 6 and sys.argv[1] == "ln_child":
    sys.path.insert(0, ROOT)
    M_, N_, K_ = (int(v) for v in sys.argv[2:5])
    torch.save(_ln_case(torch.device("cuda:0"), M_, N_, K_), sys.argv[5])
