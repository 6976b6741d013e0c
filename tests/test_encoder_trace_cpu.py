"""The three encoder towers issue the recorded launches: same order, operand geometry, scalar arguments and operand contents.

tests/golden/encoder_trace.npz was written by tests/golden/make_encoder_trace.py from instantir_amd/encoders.py as it stood
before the towers got one block packer and one block loop (the commit id is in the file).  The replay needs no GPU: `ops` is a
recording object and every weight is a small integer, so the digests do not depend on the CPU either."""
import numpy as np

from golden import make_encoder_trace as maker


def test_encoder_launch_trace_matches_the_recorded_towers():
    want = dict(np.load(maker.PATH))
    recorded_by = bytes(want.pop(maker.PARENT_KEY)).decode()
    got = maker.replay()
    assert sorted(got) == sorted({k.split("/")[0] for k in want}), "the replayed cases are not the recorded ones"
    assert len(want) == 3 * len(got)
    bad = {}
    for case in sorted(got):
        why = maker.first_difference(got[case], want[case + "/launches"], want[case + "/returned"])
        if why:
            bad[case] = why + f" (recorded ops: {bytes(want[case + '/ops']).decode()})"
    assert not bad, f"{len(bad)}/{len(got)} cases differ from the towers of commit {recorded_by}: {bad}"
    assert all(len(v[1]) >= 11 for v in got.values())          # at least two patch GEMMs, the pre-LN and one block of 8 launches
