"""CPU: which launches the chooser of csrc/gemm_conv.hip (`gemm8_auto`) sends to the 8-wave kernel of csrc/gemm8.hip, through
`iir_gemm_resolve_tile` (nothing is launched, no GPU is touched).  91 = its 256 x 320 build, 92 = its 256 x 256 build.

The ids under "keeps" were recorded by running these same queries on the library of the parent commit (a1c24a3): the 256 x 256
rule must move the Aggregator's level-2 fused q|k|v projection (4096 x 3840 x 1280, LayerNorm folded in, V written transposed)
and nothing else."""
import ctypes

import pytest

from instantir_amd import lib


@pytest.fixture(scope="module")
def h():
    h = ctypes.CDLL(lib.LIB_PATH)
    ret, args = lib.SIGNATURES["iir_gemm_resolve_tile"]
    h.iir_gemm_resolve_tile.restype, h.iir_gemm_resolve_tile.argtypes = ret, args
    return h


def _desc(M, N, K, geglu=False, ln_in=False, tr_from=None, ln_out=False, gn_out=False):
    """a descriptor as ops.gemm fills it; the addresses are never dereferenced"""
    d = lib.GemmDesc()
    d.A, d.W, d.C, d.bias = 1 << 20, 2 << 20, 3 << 20, 4 << 20
    d.M, d.N, d.K, d.lda = M, N, K, K
    d.epi, d.out_scale = (lib.EPI_GEGLU if geglu else lib.EPI_PLAIN), 1.0
    d.ldc = N // 2 if geglu else (tr_from if tr_from is not None else N)
    if ln_in:
        d.ln_stats_in, d.ln_colsum, d.ln_parts, d.ln_part_cols, d.ln_eps = 5 << 20, 6 << 20, 8, K // 8, 1e-5
    if tr_from is not None:
        d.Ct, d.ldct, d.tr_from = 7 << 20, M, tr_from
    if ln_out:
        d.ln_stats_out = 8 << 20
    if gn_out:
        d.gn_stats_out = 9 << 20
    return d


def _id(h, *a, **kw):
    return h.iir_gemm_resolve_tile(ctypes.byref(_desc(*a, **kw)))


def test_level2_aggregator_qkv_takes_the_256x256_build(h):
    assert _id(h, 4096, 3840, 1280, ln_in=True, tr_from=2560) == 92


@pytest.mark.parametrize("M,N,K", [(2048, 10240, 1280), (4096, 10240, 1280), (8192, 5120, 640), (16384, 5120, 640)])
def test_geglu_projections_stay_on_the_256x320_build(h, M, N, K):
    assert _id(h, M, N, K, geglu=True, ln_in=True) == 91
    assert _id(h, M, N, K, geglu=True) == 91


# fused q|k|v projections (ln_in, V transposed from 2N/3) and plain linears that keep the id the parent commit gives them
@pytest.mark.parametrize("M,N,K,qkv,parent_id", [
    (2048, 3840, 1280, True, 21),          # 8 x 15 = 120 tiles of 256 x 256: half a round
    (8192, 1920, 640, True, 21),           # 240 tiles, but N % 256 != 0 and K = 640
    (16384, 1920, 640, True, 91),          # 64 x 6 = 384 tiles of 256 x 320: the 320 rule, as before
    (4096, 1280, 1280, False, 54),         # 80 tiles; the 128 x 160 loader-wave build
    (4096, 3840, 640, True, 21),           # 240 tiles with K = 640: below the K bound
    (4096, 3840, 1280, False, 21),         # the same shape as a plain linear layer: not the measured form
])
def test_other_shapes_keep_their_parent_ids(h, M, N, K, qkv, parent_id):
    kw = dict(ln_in=True, tr_from=2 * N // 3) if qkv else {}
    assert _id(h, M, N, K, **kw) == parent_id


@pytest.mark.parametrize("what,parent_id", [("ln_out", 21), ("gn_out", 21), ("ragged", 21), ("res", 21), ("ct_unaligned", 21)])
def test_what_gemm8_covers_refuses_keeps_its_parent_id(h, what, parent_id):
    """4096 x 3840 x 1280 in a form the 8-wave kernel does not cover.  (LayerNorm / GroupNorm partials cannot go with a
    transposed range at all, so those two are plain launches; the others are the q|k|v form.)"""
    if what in ("ln_out", "gn_out"):
        d = _desc(4096, 3840, 1280, **{what: True})
    else:
        d = _desc(4096 - 64 if what == "ragged" else 4096, 3840, 1280, ln_in=True, tr_from=2560)
        if what == "res":
            d.res, d.ldr = 10 << 20, 2560
        if what == "ct_unaligned":
            d.ldct = 4096 + 4
    assert h.iir_gemm_resolve_tile(ctypes.byref(d)) == parent_id
