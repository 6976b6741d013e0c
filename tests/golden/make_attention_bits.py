"""Bits of the attention launches, recorded through `ops.attention`.

    python tests/golden/make_attention_bits.py <commit id of the recording checkout> [path]      # on an MI355X

`replay()` launches every build of `attn_kernel2` that `launch_attn()` in csrc/attention.hip can pick (every tile requested at
entry, the two-buffer ring built for 2 and for 3 waves per SIMD, and the identity form of each) and both builds of
`attn_hd_kernel` (head dim 80, 104), with every masked path: ragged last key tile, ragged last query tile, causal, two segments,
pre-scaled Q, fp8 output.  Q, K and V^T are slices of wider buffers with finite random borders; every output buffer is
allocated wider and longer than the view the launch writes and pre-filled with a constant, and what is stored is the SHA-256
of the WHOLE buffer, so a changed bit and a stray write both show.

The committed attention_bits.npz is never written by the code under test: it was written by the library built from the parent
of the commit that gave the two attention files one definition of their shared code (csrc/attn_geo.h), in a separate checkout
of that parent with this file copied in; the parent's commit id is stored under `PARENT_KEY`.  The recorder replays twice and
refuses to write unless both passes agree.  tests/test_kernels_gpu.py replays the cases on the current library and asserts
equality, key for key.

Shapes: the smallest that reach every build (see `launch_attn`: <= 4 key tiles in all and not causal -> staged at entry;
otherwise the ring, for 3 waves per SIMD above 512 attending workgroups).
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "attention_bits.npz")
PARENT_KEY = "recorded_by_commit"

FILL = 7.0
BORDER = 8
LOG2E = 1.4426950408889634

# (key, head dim, batch, heads, Tq, [Tkv per segment], options)
CASES = [
    # d64, every tile requested at entry: text + IP cross-attention, ragged last query tile
    ("d64.pre.2seg", 64, 2, 2, 192, [77, 64], {}),
    ("d64.pre.2seg.qpre", 64, 2, 2, 192, [77, 64], dict(q_prescaled=True)),
    ("d64.pre.2seg.o_fp8", 64, 2, 2, 192, [77, 64], dict(o_fp8=True)),
    # d64, two-buffer ring built for 2 waves per SIMD: five tiles with a ragged tail of 44; the CLIP text encoders' causal form
    ("d64.ring2.t300", 64, 2, 2, 300, [300], {}),
    ("d64.ring2.causal77", 64, 2, 2, 77, [77], dict(causal=True, kv_rows=80)),
    ("d64.ring2.causal80over77", 64, 2, 2, 80, [77], dict(causal=True, kv_rows=80)),       # as HipCLIPText launches it
    # d64, ring built for 3 waves per SIMD: 16 query tiles x 33 pairs = 528 workgroups, six key tiles with a ragged tail
    ("d64.ring3.t2048x330", 64, 3, 11, 2048, [330], {}),
    # d64, identity form of each build
    ("d64.ident.pre.t192", 64, 3, 2, 192, [192], dict(ident_from=2)),
    ("d64.ident.ring2.t320", 64, 3, 2, 320, [320], dict(ident_from=2)),
    ("d64.ident.ring3.t2048", 64, 4, 11, 2048, [2048], dict(ident_from=3)),
]
for _D in (80, 104):
    CASES += [
        (f"d{_D}.ragged.100x77", _D, 1, 3, 100, [77], {}),
        (f"d{_D}.ragged.33x1", _D, 2, 2, 33, [1], {}),
        (f"d{_D}.ragged.130x131", _D, 1, 2, 130, [131], {}),
        (f"d{_D}.causal77", _D, 2, 2, 77, [77], dict(causal=True)),
        (f"d{_D}.2seg", _D, 2, 2, 100, [13, 16], {}),
        (f"d{_D}.qpre", _D, 1, 2, 200, [200], dict(q_prescaled=True)),
    ]


def replay():
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from instantir_amd import lib, ops
    lib.load()
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(20261017)
    out = {}

    def rand(*shape, scale=1.0):
        return torch.from_numpy((rng.standard_normal(shape) * scale).astype(np.float32)).half().to(dev)

    for key, D, B, heads, Tq, tkvs, opt in CASES:
        C = heads * D
        scale = D ** -0.5
        qb = rand(B * Tq, C + 2 * BORDER)                        # Q, K: column slices of wider buffers
        if opt.get("q_prescaled"):
            qb = (qb.float() * (scale * LOG2E)).half()
        kv = []
        for tkv in tkvs:
            rows = opt.get("kv_rows", tkv)                      # rows of one batch entry of K; V^T columns likewise
            tpad = (rows + 7) // 8 * 8
            kb = rand(B * rows, C + 2 * BORDER)
            vb = rand(C + 2 * BORDER, B * tpad + 64)            # V^T: row slice; random columns past the last batch entry
            for b in range(B):
                vb[:, b * tpad + tkv:(b + 1) * tpad] = 0         # contract: finite on [0, roundup8(Tkv)); zero past Tkv
            kv.append((kb[:, BORDER:BORDER + C], rows, vb[BORDER:BORDER + C], tpad, tkv))
        dtype = torch.uint8 if opt.get("o_fp8") else torch.float16
        big = torch.full((B * Tq + 3, C + 8), FILL, dtype=dtype, device=dev)      # 3 rows and 8 columns of margin
        ops.attention(qb[:, BORDER:BORDER + C], big[:B * Tq, :C], kv, B, heads, Tq, scale=scale, causal=opt.get("causal", False),
                      q_prescaled=opt.get("q_prescaled", False), head_dim=D, ident_from=opt.get("ident_from", 0))
        torch.cuda.synchronize()
        if dtype == torch.float16:
            assert torch.isfinite(big).all(), key
        assert key not in out, key
        out[key] = np.frombuffer(hashlib.sha256(big.contiguous().view(torch.uint8).cpu().numpy().tobytes()).digest(), dtype=np.uint8)
    return out


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    path = sys.argv[2] if len(sys.argv) > 2 else PATH
    bits, again = replay(), replay()
    differ = [k for k in bits if not np.array_equal(bits[k], again[k])]
    if differ:
        sys.exit(f"two recordings differ: {differ}")
    bits[PARENT_KEY] = np.frombuffer(sys.argv[1].encode(), dtype=np.uint8)
    np.savez_compressed(path, **bits)
    print(f"wrote {path}: {len(bits) - 1} buffers recorded twice by {sys.argv[1]}, {os.path.getsize(path)} bytes")
