"""Bits of what the three encoder towers return, recorded through their public surface.

    python tests/golden/make_encoder_bits.py <commit id of the recording checkout> [path]      # on an MI355X

`replay()` runs every case of tests/golden/encoder_cases.py on cuda:0 with fp16-representable random-normal weights (norms
perturbed, LayerScale in [0.5, 1]) and returns {key: SHA-256 of the returned tensor's bytes}: DINOv2 with the native and the
bicubic position table, the CLIP vision tower at head dims 64 / 80 / 104 with both activations and with `image_embeds`, the
CLIP text tower with both activations and eos rules, `clip_skip` and `text_embeds`, and both outputs of `encode_image_pair`.

The committed encoder_bits.npz is never written by the code under test: it was written on the tree whose
instantir_amd/encoders.py and library were still those of the parent of the commit that gave the three towers one block
packer and one block loop; the parent's commit id is stored under `PARENT_KEY`.  The recorder replays twice and refuses to
write unless both passes agree.  tests/test_encoder_bits_gpu.py replays the cases on the current code and asserts equality,
key for key.
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "encoder_bits.npz")
PARENT_KEY = "recorded_by_commit"


def replay():
    import torch
    sys.path[:0] = [p for p in (os.path.dirname(os.path.dirname(HERE)), HERE) if p not in sys.path]
    import encoder_cases as EC
    from instantir_amd import lib
    lib.load()
    out = {}
    for case, call in EC.cases(EC.draw_normal, torch.device("cuda:0")):
        for name, t in call().items():
            if t is None:                                   # a text tower without text_projection has no pooled output
                continue
            torch.cuda.synchronize()
            assert torch.isfinite(t).all(), (case, name)
            key = f"{case}.{name}"
            assert key not in out, key
            out[key] = np.frombuffer(hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).digest(), dtype=np.uint8)
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
    print(f"wrote {path}: {len(bits) - 1} tensors recorded twice by {sys.argv[1]}, {os.path.getsize(path)} bytes")
