"""GPU: the input pipeline (csrc/preprocess.hip, csrc/video_tail.hip) writes, bit for bit, what the library before the
layout / table / dispatch refactor wrote: tests/golden/preprocess_parent_digests.json holds the SHA-256 of every output
of tests/gen_preprocess_digests.py, recorded on an MI355X from that earlier library, and this file recomputes them.

A mismatch means an arithmetic expression, a summation order or an output index moved.  The golden file is never
re-recorded from the tree under test to make this pass.  A later change that MEANS to change some of these bits (a new
filter, another rounding) regenerates it on purpose: check out the commit before that change, build it, run
`python tests/gen_preprocess_digests.py` there on an MI355X, copy the JSON here, then show in the change itself which
cases moved and why; cases that were not meant to move must still match the old file.
"""
import json

import pytest
import torch

import gen_preprocess_digests as gen

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def got(pkg, hiplib):
    assert torch.cuda.is_available()
    return gen.digests(pkg)


@pytest.fixture(scope="module")
def want():
    with open(gen.OUT) as f:
        return json.load(f)


def test_the_same_cases_are_digested(got, want):
    assert sorted(got) == sorted(want)


@pytest.mark.parametrize("family", ["fwd", "aug", "views", "views_bwd", "bwd", "video_tail"])
def test_outputs_match_the_parent_library_bit_for_bit(got, want, family):
    names = [n for n in want if n.split("/")[0] == family]
    assert names, family
    moved = [n for n in names if got.get(n) != want[n]]
    print(f"[digests] {family}: {len(names) - len(moved)}/{len(names)} match")
    assert not moved, f"{len(moved)} of {len(names)} outputs differ from the parent library: {moved[:8]}"
