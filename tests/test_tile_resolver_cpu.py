"""CPU: the one tile resolver of csrc/gemm_conv.hip, through the C ABI, over the GEMM / conv shapes of the 1024x1024 step (main
and previewer UNets, Aggregator; 2 rows).  The queries a step is planned with -- `iir_gemm_gn_supported`, `iir_gemm_ln_parts` --
must agree with the launch `iir_gemm_resolve_tile` names; the 257-512-tile problems of 64x160 with K >= 1280 resolve to the
128x160 loader-wave build (id 54); with IIR_T4_LW=0 every shape resolves to what the round-3 selection chose.  The switches are
read once per process, so each setting is evaluated in a fresh child process (no GPU is touched: nothing is launched)."""
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BM = {1: 128, 2: 128, 3: 64, 4: 128, 5: 64}
BN = {1: 128, 2: 64, 3: 64, 4: 160, 5: 160}


def step_shapes():
    """(M, N, K, conv) of the step's launches (a superset: every projection / conv family at every level)"""
    R = 2
    out = set()
    levels = [(128 * 128, 320), (64 * 64, 640), (32 * 32, 1280)]               # UNets
    levels += [(256 * 128, 320), (128 * 64, 640), (64 * 32, 1280)]             # Aggregator: 2H x W inputs
    for hw, C in levels:
        M = R * hw
        for N, K in ((C, C), (3 * C, C), (8 * C, C), (C, 4 * C), (2 * C, C), (C, 2 * C)):
            out.add((M, N, K, False))
        for cin in (C // 2, C, 3 * C // 2, 2 * C, 3 * C, 4 * C):             # 3x3 convs, skip-concat inputs included
            if cin % 64 == 0:
                out.add((M, C, 9 * cin, True))
                out.add((M // 4, C, 9 * cin, True))                              # stride-2 downsample
                out.add((M, C, cin, True))                                       # 1x1 shortcuts
        out.add((M, 2 * C, 9 * C, True))                                         # SFT gamma | beta
    for K in (2048, 1280):                                                     # text / IP keys and values, time embeddings
        for N in (640, 1280, 2560):
            out.add((R * 77, N, K, False))
            out.add((R * 16, N, K, False))
    return sorted(out)


def in_scope(M, N, K):
    return K >= 1280 and M % 128 == 0 and N % 160 == 0 and (M // 128) * (N // 160) <= 256 < (M // 64) * (N // 160)


def round3_id(h, M, N, K):
    """the round-3 selection (4-wave kernel, default switches): pick_tile's shape, 3-stage loader waves one per CU"""
    base = h.iir_gemm_pick_tile(M, N, K, 0)
    blocks = -(-M // BM[base]) * -(-N // BN[base])
    return 55 if base == 5 and blocks <= 256 and K >= 1280 else base + 20


def _resolve_all():
    sys.path.insert(0, ROOT)
    from instantir_amd import lib
    h = ctypes.CDLL(lib.LIB_PATH)
    for name in ("iir_gemm_pick_tile", "iir_gemm_gn_supported", "iir_gemm_ln_parts", "iir_gemm_resolve_tile", "iir_gemm_tile_bn"):
        ret, args = lib.SIGNATURES[name]
        getattr(h, name).restype, getattr(h, name).argtypes = ret, args
    rows = []
    for M, N, K, conv in step_shapes():
        d = lib.GemmDesc()
        d.A, d.W, d.C = 1 << 20, 2 << 20, 3 << 20           # never dereferenced: nothing is launched
        d.lda, d.ldc, d.M, d.N, d.K = K, N, M, N, K
        rows.append(dict(M=M, N=N, K=K, conv=conv, id=h.iir_gemm_resolve_tile(ctypes.byref(d)), gn=h.iir_gemm_gn_supported(M, N, K, int(conv)),
                         ln=h.iir_gemm_ln_parts(M, N, K), bn=None, round3=round3_id(h, M, N, K)))
        rows[-1]["bn"] = h.iir_gemm_tile_bn(rows[-1]["id"])
    return rows


def _child(t4_lw):
    env = {k: v for k, v in os.environ.items() if not k.startswith("IIR_")}
    if t4_lw is not None:
        env["IIR_T4_LW"] = t4_lw
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


def _consistent(rows):
    for r in rows:
        M, N, K, t = r["M"], r["N"], r["K"], r["id"]
        if t == 91:                                          # a GEMM of this shape takes the 8-wave 256x320 kernel (gemm8.hip)
            continue
        bm, bn = BM[t % 10], BN[t % 10]
        assert r["bn"] == bn, r
        whole = M % bm == 0 and N % bn == 0
        assert r["gn"] == int(M % 64 == 0 and whole), r
        if not r["conv"]:
            assert r["ln"] == (N // bn if whole and N // bn <= 8 else 0), r


def test_resolver_agrees_with_its_queries_and_takes_the_new_tile():
    rows = _child(None)
    _consistent(rows)
    scope = [r for r in rows if in_scope(r["M"], r["N"], r["K"])]
    assert {(r["M"], r["N"]) for r in scope} >= {(4096, 1280), (8192, 640)}
    for r in rows:
        if r["id"] == 91:
            continue
        want = 54 if in_scope(r["M"], r["N"], r["K"]) else r["round3"]
        assert r["id"] == want, r


def test_switch_off_restores_the_round3_ids():
    rows = _child("0")
    _consistent(rows)
    for r in rows:
        assert r["id"] != 54 and (r["id"] == 91 or r["id"] == r["round3"]), r


if __name__ == "__main__":
    print(json.dumps(_resolve_all()))
