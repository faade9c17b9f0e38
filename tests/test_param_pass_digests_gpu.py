"""GPU: the parameter-side passes (gradient norm, EMA, AdamW with its weight shadows, the weight re-cast, the bf16x3
operand split) write, bit for bit, what the library before the placement-table / tile-writer / chunk-walk refactor
wrote: tests/golden/param_pass_parent_digests.json holds the SHA-256 of every output of tests/gen_param_pass_digests.py,
recorded on an MI355X from that earlier library, and this file recomputes them.

A mismatch means an arithmetic expression, a summation order, a store condition or a destination offset moved.  The golden
file is never re-recorded from the tree under test to make this pass.  A later change that MEANS to change some of these
bits regenerates it on purpose: check out the commit before that change, build it, run
`python tests/gen_param_pass_digests.py` there on an MI355X, copy the JSON here, then show in the change itself which cases
moved and why; cases that were not meant to move must still match the old file.
"""
import json

import pytest
import torch

import gen_param_pass_digests as gen

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


@pytest.mark.parametrize("family", ["table", "tiled", "model", "cast_job", "split3"])
def test_outputs_match_the_parent_library_bit_for_bit(got, want, family):
    names = [n for n in want if n.split("/")[0] == family]
    assert names, family
    moved = [n for n in names if got.get(n) != want[n]]
    print(f"[digests] {family}: {len(names) - len(moved)}/{len(names)} match")
    assert not moved, f"{len(moved)} of {len(names)} outputs differ from the parent library: {moved[:8]}"


def test_the_two_routes_agree_within_this_tree(got):
    """sgl_op_grad_norm is sgl_op_grad_norm_scaled at scale 1, bit for bit; and the shadow arena the optimizer wrote in its
    own pass is, byte for byte (padding and the gaps between allocations included), the arena a fresh re-cast of the same
    parameters writes."""
    pairs = gen.twins(got)
    assert len(pairs) == len(gen.MAX_NORMS) + 2 * len(gen.MODEL_CONFIGS) * len(gen.TRAIN_MODES)
    apart = [(a, b) for a, b in pairs if got[a] != got[b]]
    assert not apart, f"{len(apart)} of {len(pairs)} pairs differ: {apart[:4]}"
