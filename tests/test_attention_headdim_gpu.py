"""GPU: `ops.attention(head_dim=80 / 104)` (`iir_attention_f16`, the CLIP ViT-H/14 and bigG/14 vision towers) against fp32
SDPA.  Every case runs with NaN in the memory around its operands -- the columns beside Q / K, the V^T rows beside the heads
and the V^T columns past the last batch -- and a sentinel around O, so a read or write outside the contract shows."""
import pytest
import torch

pytestmark = pytest.mark.gpu

LOG2E = 1.4426950408889634
SENTINEL = 7.0


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from instantir_amd import lib
    lib.load()
    return torch.device("cuda:0")


def _rand(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).half()


def _close(got, want, rtol=3e-3, atol=3e-3, what=""):
    got = got.float().cpu()
    err = (got - want).abs()
    bad = (err > atol + rtol * want.abs()).sum().item()
    assert bad == 0, f"{what}: {bad}/{want.numel()} off, max err {err.max().item():.4g} (ref max {want.abs().max().item():.4g})"


def _sdpa_ref(q, k, v, heads, D, causal=False):
    b, tq, _ = q.shape
    sp = lambda x: x.float().reshape(b, x.shape[1], heads, D).transpose(1, 2)
    s = sp(q) @ sp(k).transpose(-1, -2) * D ** -0.5
    if causal:
        s = s.masked_fill(torch.ones(tq, k.shape[1], dtype=torch.bool).triu(1), float("-inf"))
    return (torch.softmax(s, dim=-1) @ sp(v)).transpose(1, 2).reshape(b, tq, heads * D)


def _launch(dev, D, B, heads, q, segs, causal=False, q_prescaled=False, border=8):
    """q (B, Tq, C) fp16 host; segs: list of (k, v) host (B, Tkv, C).  Q / K are column slices of NaN-bordered buffers, V^T a
    row slice of a NaN-bordered one with NaN columns past the last batch, O a column slice of a sentinel-filled buffer.
    Returns (O view, O buffer)."""
    from instantir_amd import ops
    C, Tq = heads * D, q.shape[1]
    nan = float("nan")
    qb = torch.full((B * Tq, C + 2 * border), nan, dtype=torch.half, device=dev)
    qb[:, border:border + C] = q.reshape(-1, C).to(dev)
    kv = []
    for k, v in segs:
        tkv = k.shape[1]
        tpad = (tkv + 7) // 8 * 8
        kb = torch.full((B * tkv, C + 2 * border), nan, dtype=torch.half, device=dev)
        kb[:, border:border + C] = k.reshape(-1, C).to(dev)
        vb = torch.full((C + 2 * border, B * tpad + 64), nan, dtype=torch.half, device=dev)
        for b in range(B):
            vb[border:border + C, b * tpad:(b + 1) * tpad] = 0          # contract: finite on [0, roundup8(Tkv))
            vb[border:border + C, b * tpad:b * tpad + tkv] = v[b].T.to(dev)
        kv.append((kb[:, border:border + C], tkv, vb[border:border + C], tpad, tkv))
    ob = torch.full((B * Tq, C + 2 * border), SENTINEL, dtype=torch.half, device=dev)
    o = ob[:, border:border + C]
    ops.attention(qb[:, border:border + C], o, kv, B, heads, Tq, scale=D ** -0.5, causal=causal, q_prescaled=q_prescaled,
                  head_dim=D)
    torch.cuda.synchronize()
    return o, ob


def _check_border(ob, C, border=8):
    assert (ob[:, :border] == SENTINEL).all() and (ob[:, border + C:] == SENTINEL).all(), "O written outside [0, heads*D)"


def _case(dev, D, B, heads, Tq, Tkv, seed, causal=False):
    g = torch.Generator().manual_seed(seed)
    C = heads * D
    q, k, v = _rand(g, B, Tq, C), _rand(g, B, Tkv, C), _rand(g, B, Tkv, C)
    o, ob = _launch(dev, D, B, heads, q, [(k, v)], causal=causal)
    assert torch.isfinite(o).all()
    _close(o, _sdpa_ref(q, k, v, heads, D, causal).reshape(B * Tq, C), what=f"D={D} B={B} h={heads} Tq={Tq} Tkv={Tkv}")
    _check_border(ob, C)


@pytest.mark.parametrize("D", [80, 104])
def test_tower_self_attention(dev, D):
    """ViT-H/14 / bigG/14 at 224 px: 2 images, 16 heads, 257 tokens."""
    _case(dev, D, 2, 16, 257, 257, seed=D)


@pytest.mark.parametrize("D", [80, 104])
@pytest.mark.parametrize("B,heads,Tq,Tkv", [(1, 3, 100, 77), (2, 2, 33, 1), (1, 2, 130, 131), (2, 1, 7, 65), (1, 2, 256, 200)])
def test_ragged_shapes(dev, D, B, heads, Tq, Tkv):
    """Tq != Tkv, a single key, and lengths that are not multiples of 8 or 64."""
    _case(dev, D, B, heads, Tq, Tkv, seed=D + Tq + Tkv)


@pytest.mark.parametrize("D", [80, 104])
def test_causal(dev, D):
    _case(dev, D, 2, 2, 77, 77, seed=D + 77, causal=True)


@pytest.mark.parametrize("D", [80, 104])
def test_two_segments(dev, D):
    """13 + 16 keys sharing one query, outputs summed."""
    g = torch.Generator().manual_seed(D + 21)
    B, heads, Tq = 2, 2, 100
    C = heads * D
    q = _rand(g, B, Tq, C)
    k1, v1, k2, v2 = _rand(g, B, 13, C), _rand(g, B, 13, C), _rand(g, B, 16, C), _rand(g, B, 16, C)
    o, ob = _launch(dev, D, B, heads, q, [(k1, v1), (k2, v2)])
    want = _sdpa_ref(q, k1, v1, heads, D) + _sdpa_ref(q, k2, v2, heads, D)
    _close(o, want.reshape(B * Tq, C), what=f"two segments D={D}")
    _check_border(ob, C)


@pytest.mark.parametrize("D", [80, 104])
def test_q_prescaled(dev, D):
    """Q already holds q * scale * log2(e): the kernel uses it as it stands."""
    g = torch.Generator().manual_seed(D + 5)
    B, heads, T = 1, 2, 200
    C = heads * D
    c = D ** -0.5 * LOG2E
    q, k, v = _rand(g, B, T, C), _rand(g, B, T, C), _rand(g, B, T, C)
    qp = (q.float() * c).half()
    o, ob = _launch(dev, D, B, heads, qp, [(k, v)], q_prescaled=True)
    _close(o, _sdpa_ref(qp.float() / c, k, v, heads, D).reshape(B * T, C), what=f"q_prescaled D={D}")
    _check_border(ob, C)


@pytest.mark.parametrize("D", [80, 104])
def test_online_softmax_rescale(dev, D):
    """One key far above the rest sits in the last tile: the running maximum grows late."""
    g = torch.Generator().manual_seed(D + 2)
    B, heads, T = 1, 1, 256
    q, k, v = _rand(g, B, T, D), _rand(g, B, T, D), _rand(g, B, T, D)
    k[0, 250] = q[0, 3] * 4.0
    o, ob = _launch(dev, D, B, heads, q, [(k, v)])
    _close(o, _sdpa_ref(q, k, v, heads, D).reshape(T, D), what=f"rescale D={D}")
    _check_border(ob, D)


@pytest.mark.parametrize("D", [80, 104])
def test_large_grid(dev, D):
    """T = 4096, B = 2, 16 heads: one (batch, head) pair against SDPA, every pair equal to it (same inputs everywhere)."""
    from instantir_amd import ops
    g = torch.Generator().manual_seed(D + 4096)
    B, heads, T = 2, 16, 4096
    C = heads * D
    pair = _rand(g, 3, T, D)
    q = pair[0].repeat(B, heads).reshape(B * T, C).contiguous().to(dev)
    k = pair[1].repeat(B, heads).reshape(B * T, C).contiguous().to(dev)
    vt = pair[2].T.contiguous().repeat(heads, B).to(dev)
    o = torch.empty(B * T, C, dtype=torch.half, device=dev)
    ops.attention(q, o, [(k, T, vt, T, T)], B, heads, T, scale=D ** -0.5, head_dim=D)
    torch.cuda.synchronize()
    want = _sdpa_ref(pair[0][None], pair[1][None], pair[2][None], 1, D).reshape(T, D)
    got = o.reshape(B, T, heads, D)
    _close(got[0, :, 0], want, what=f"T=4096 D={D}")
    for b in range(B):
        for h in range(heads):
            assert torch.equal(got[b, :, h], got[0, :, 0]), "identical (batch, head) pairs gave different outputs"


@pytest.mark.parametrize("D", [80, 104])
def test_neighbour_safety_wide_borders(dev, D):
    """A whole head's width of NaN on either side of Q / K / V^T and of sentinel around O (the tower's fused q|k buffer puts
    K right after Q): the result is finite and correct, and nothing outside [0, heads*D) of O is written."""
    g = torch.Generator().manual_seed(D + 9)
    B, heads, T = 2, 4, 100
    C = heads * D
    q, k, v = _rand(g, B, T, C), _rand(g, B, T, C), _rand(g, B, T, C)
    o, ob = _launch(dev, D, B, heads, q, [(k, v)], border=104)
    assert torch.isfinite(o).all()
    _close(o, _sdpa_ref(q, k, v, heads, D).reshape(B * T, C), what=f"wide borders D={D}")
    _check_border(ob, C, border=104)


@pytest.mark.parametrize("D", [80, 104])
def test_repeatable(dev, D):
    """Two identical calls give bit-identical outputs."""
    g = torch.Generator().manual_seed(D + 3)
    B, heads, T = 2, 16, 257
    C = heads * D
    q, k, v = _rand(g, B, T, C), _rand(g, B, T, C), _rand(g, B, T, C)
    o1, _ = _launch(dev, D, B, heads, q, [(k, v)])
    o2, _ = _launch(dev, D, B, heads, q, [(k, v)])
    assert torch.equal(o1, o2)


def test_other_head_dims_are_refused(dev):
    from instantir_amd import lib, ops
    q = torch.zeros(16, 2 * 96, dtype=torch.half, device=dev)
    vt = torch.zeros(2 * 96, 16, dtype=torch.half, device=dev)
    for hd in (96, 128):
        with pytest.raises(lib.HipLibraryError):
            ops.attention(q, torch.empty_like(q), [(q, 16, vt, 16, 16)], 1, 2, 16, head_dim=hd)
