"""GPU: the bits of the image-scoring and resampling kernels against the library as it stood before they shared
csrc/image_common.h (tests/golden/scoring_bits.npz, written by tests/golden/make_scoring_bits.py)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from instantir_amd import lib
    lib.load()
    return torch.device("cuda:0")


def test_scoring_bits_match_the_recorded_library(dev, golden_dir):
    """Every output of ops.image_metrics, niqe_stats, lpips_prep, lpips_tap and resample, replayed on seeded inputs at the
    smallest shapes that reach each kernel's partial tiles, remainder quads and every lane-group width, as integer views (a NaN
    column compares as its bits): a reordered sum or a regrouped statement shows here, where the fp64 restatements of the other
    GPU tests allow it within their tolerances."""
    from golden.make_scoring_bits import replay
    want = np.load(os.path.join(golden_dir, "scoring_bits.npz"))
    got = replay()
    assert sorted(got) == sorted(want.files)
    bad = [k for k in want.files if got[k].dtype != want[k].dtype or not np.array_equal(got[k], want[k])]
    assert not bad, bad
