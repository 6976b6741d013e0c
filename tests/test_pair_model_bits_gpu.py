"""GPU: the bits of LPIPS, DISTS and the metrics calls that score with them against the tree as it stood before the two models
shared instantir_amd/vgg.py (tests/golden/pair_model_bits.npz, written by tests/golden/make_pair_model_bits.py)."""
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


def test_pair_model_bits_match_the_recorded_tree(dev, golden_dir):
    """Every output of both models (LPIPS: the (N, 5) terms and all five maps; DISTS: the score and its (N, 6, 2) terms) for
    uint8, fp32 and mixed pairs at 17 x 19 in both 16-bit types, the wide network at 33 x 18, and the results of
    metrics.evaluate / metrics.input_fidelity with both models given (keys in order, values as float bits, a refusal as its
    text), as integer views."""
    from golden.make_pair_model_bits import replay
    want = np.load(os.path.join(golden_dir, "pair_model_bits.npz"))
    got = replay()
    assert sorted(got) == sorted(want.files)
    bad = [k for k in want.files if got[k].dtype != want[k].dtype or not np.array_equal(got[k], want[k])]
    assert not bad, bad
