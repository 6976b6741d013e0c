"""Generate tests/golden/freeu.npz by RUNNING the reference's own FreeU code (module/min_sdxl.py:22-77:
`fourier_filter`, `apply_freeu`) on seeded inputs.

Run in the build container only (needs the reference checkout that make_reference_goldens.py points at):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_freeu_golden.py

`module.min_sdxl` imports diffusers' attention processors; the same import shim as make_reference_goldens.py
(re-exports of the reference's own classes, no arithmetic) makes it importable.  Every output number is computed by
the reference functions in fp32.

Contents, per shape tag `HxW`: `HxW.hidden` (1, 2, H, W) and `HxW.skip` (1, 2, H, W) inputs (fp16 values stored as fp16),
and for resolution_idx i in (0, 1): `HxW.hidden_out{i}` / `HxW.skip_out{i}` (fp32), with s1, s2, b1, b2 = FACTORS.
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import make_reference_goldens as MRG  # noqa: E402  (puts the reference on sys.path)

SHAPES = [(32, 32), (64, 64), (24, 32), (5, 7), (2, 2), (1, 4)]
FACTORS = (0.9, 0.2, 1.3, 1.4)          # s1, s2, b1, b2 (diffusers' SDXL values)


def main():
    MRG._install_diffusers_shim()
    MRG._extend_shim_for_min_sdxl_and_aggregator()
    from module import min_sdxl

    s1, s2, b1, b2 = FACTORS
    g = torch.Generator().manual_seed(20261015)
    out = {"factors": np.array(FACTORS, dtype=np.float64)}
    for H, W in SHAPES:
        tag = f"{H}x{W}"
        hidden = (torch.randn(1, 2, H, W, generator=g) * 2.0 + 0.3).half()
        skip = (torch.randn(1, 2, H, W, generator=g) * 1.5 - 0.2).half()
        out[f"{tag}.hidden"] = hidden.numpy()
        out[f"{tag}.skip"] = skip.numpy()
        for idx in (0, 1):
            h, s = min_sdxl.apply_freeu(idx, hidden.float().clone(), skip.float().clone(), s1=s1, s2=s2, b1=b1, b2=b2)
            out[f"{tag}.hidden_out{idx}"] = h.numpy().astype(np.float32)
            out[f"{tag}.skip_out{idx}"] = s.numpy().astype(np.float32)
    path = os.path.join(MRG.OUT, "freeu.npz")
    np.savez_compressed(path, **out)
    print(f"{path} written ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
