"""Every output of the three encoder towers, bit for bit against the towers as they stood before they shared one block.

tests/golden/encoder_bits.npz holds the SHA-256 of every tensor the cases of tests/golden/encoder_cases.py return, written on an
MI355X by tests/golden/make_encoder_bits.py from instantir_amd/encoders.py and the library of the commit named in the file.  The
same calls on the current code must return the same bits, key for key."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_encoder_bits_match_the_recorded_towers():
    from golden import make_encoder_bits as maker
    want = dict(np.load(maker.PATH))
    recorded_by = bytes(want.pop(maker.PARENT_KEY)).decode()
    got = maker.replay()
    assert len(got) == len(want) and sorted(got) == sorted(want), "the replayed cases are not the recorded ones"
    bad = [k for k in sorted(want) if not np.array_equal(got[k], want[k])]
    assert not bad, f"{len(bad)}/{len(want)} tensors differ from the towers of commit {recorded_by}: {bad}"
