"""The launch sequence of an LPIPS pair and a DISTS pair against the tree as it stood before the two shared
instantir_amd/vgg.py (tests/golden/pair_trace.json, written by tests/golden/make_pair_trace.py).  No GPU: the ops are recorders."""
import json
import os

import pytest

from golden.make_pair_trace import SIZES, WIDTHS, replay


@pytest.fixture(scope="module")
def traces(golden_dir):
    with open(os.path.join(golden_dir, "pair_trace.json")) as f:
        return json.load(f), replay()


def test_the_cases_are_the_recorded_ones(traces):
    want, got = traces
    assert list(got) == list(want)
    assert len(want) == 2 * len(WIDTHS) * len(SIZES) * 3                 # fp16 / bf16; LPIPS without and with maps, DISTS
    assert {len(c) for k, c in want.items() if k.startswith("lpips.")} == {28}
    assert {len(c) for k, c in want.items() if k.startswith("dists.")} == {33}


def test_every_launch_of_a_pair_is_the_recorded_one(traces):
    """Op by op: the entry, and every argument by name -- a tensor as [whose storage, storage offset, shape, strides, dtype], a
    scalar as it is.  17 x 19 is where floor (LPIPS) and ceil (DISTS) halving part ways at every level; the widths
    (72, 136, 64, 8, 264) pad differently per stage."""
    want, got = traces
    for case in want:
        assert [c[0] for c in got[case]] == [c[0] for c in want[case]], case
        for n, (g, w) in enumerate(zip(got[case], want[case])):
            assert g == w, (case, n)
