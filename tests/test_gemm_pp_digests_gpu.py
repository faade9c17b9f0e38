"""GPU: the anti-phase GEMM kernels of csrc/gemm_bf16_v2.hip (256x256 and 384x192 NT tiles with every epilogue they take,
the 256x256 TN tile) write, bit for bit, what the library before the one-kernel / one-epilogue / one-launcher refactor of
that file wrote: tests/golden/gemm_pp_parent_digests.json holds the SHA-256 of every output of
tests/gen_gemm_pp_digests.py, recorded on an MI355X from that earlier library, and this file recomputes them.

A mismatch means an accumulation order, an epilogue expression, a store condition or a destination offset moved.  The
golden file is never re-recorded from the tree under test to make this pass.  A later change that MEANS to change some of
these bits regenerates it on purpose: check out the commit before that change, build it, run
`python tests/gen_gemm_pp_digests.py` there on an MI355X, copy the JSON here, then show in the change itself which cases
moved and why; cases that were not meant to move must still match the old file.
"""
import json
import os

import pytest
import torch

import gen_gemm_pp_digests as gen

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def got(hiplib):
    assert torch.cuda.is_available()
    assert "SGL_NT_TILE" not in os.environ and "SGL_BAND" not in os.environ, "the digests are those of the default dispatch"
    return gen.digests(hiplib)


@pytest.fixture(scope="module")
def want():
    with open(gen.OUT) as f:
        return json.load(f)


def test_the_same_cases_are_digested(got, want):
    assert sorted(got) == sorted(want)


@pytest.mark.parametrize("family", ["nt256", "qkv", "nt384", "tn256"])
def test_outputs_match_the_parent_library_bit_for_bit(got, want, family):
    names = [n for n in want if n.split("/")[0] == family]
    assert names, family
    moved = [n for n in names if got.get(n) != want[n]]
    print(f"[digests] {family}: {len(names) - len(moved)}/{len(names)} match")
    assert not moved, f"{len(moved)} of {len(names)} outputs differ from the parent library: {moved[:8]}"
