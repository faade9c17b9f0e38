"""GPU: the attention entry points (sgl_op_attn_fwd / _bwd, sgl_op_attn_probs, sgl_op_pool_attn_fwd / _bwd) return the
status codes and write, bit for bit, what the library before the consolidation of their host front (one shape contract,
one dispatcher, one head addressing in csrc/attention.hip.h) returned and wrote: tests/golden/attn_parent_digests.json
holds the status codes and the SHA-256 of every guarded output of tests/gen_attn_digests.py, recorded on an MI355X from
that earlier library, and this file recomputes them.

A mismatch means an accepted shape became a refused one (or the reverse), a scale constant, an accumulation order, a store
condition or a destination offset moved.  The golden file is never re-recorded from the tree under test to make this
pass.  A later change that MEANS to change some of these bits regenerates it on purpose: check out the commit before that
change, build it, run `SGL_LIB_PATH=<that build's library> python tests/gen_attn_digests.py` on an MI355X, copy the JSON
here, then show in the change itself which cases moved and why; cases that were not meant to move must still match.
"""
import json

import pytest
import torch

import gen_attn_digests as gen

pytestmark = pytest.mark.gpu
FAMILIES = ["fwdbwd", "probs", "pool", "refuse"]


@pytest.fixture(scope="module")
def clean():
    return {}


@pytest.fixture(scope="module")
def got(hiplib, clean):
    assert torch.cuda.is_available()
    return gen.digests(hiplib, clean)


@pytest.fixture(scope="module")
def want():
    with open(gen.OUT) as f:
        return json.load(f)


def test_the_same_cases_are_digested(got, want):
    assert sorted(got) == sorted(want)
    for fam in FAMILIES:
        assert any(n.split("/")[0] == fam for n in want), fam


@pytest.mark.parametrize("family", FAMILIES)
def test_status_codes_match_the_parent_library(got, want, family):
    moved = [(n, got[n]["rc"], want[n]["rc"]) for n in want if n.split("/")[0] == family and got[n]["rc"] != want[n]["rc"]]
    assert not moved, f"status codes differ from the parent library (case, got, want): {moved[:8]}"
    accepted = [n for n in want if n.split("/")[0] == family and any(want[n]["rc"])] if family != "refuse" else []
    assert not accepted, f"cases that are there for their outputs were refused: {accepted[:8]}"


@pytest.mark.parametrize("family", FAMILIES)
def test_outputs_match_the_parent_library_bit_for_bit(got, want, family):
    names = [n for n in want if n.split("/")[0] == family]
    moved = [n for n in names if got[n]["sha"] != want[n]["sha"]]
    print(f"[attn digests] {family}: {len(names) - len(moved)}/{len(names)} match")
    assert not moved, f"{len(moved)} of {len(names)} outputs differ from the parent library: {moved[:8]}"


def test_refused_calls_refuse_and_leave_their_outputs_untouched(got, clean):
    names = [n for n in got if n.startswith("refuse/")]
    assert names and sorted(names) == sorted(clean)
    passed = [n for n in names if not all(got[n]["rc"])]
    assert not passed, f"accepted: {passed}"
    written = [n for n in names if got[n]["sha"] != clean[n]]
    assert not written, f"a refused call wrote its outputs: {written}"
