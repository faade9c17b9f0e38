"""Host: sgl_adamw_bind_shadows binds, field for field, what the library before the placement-table refactor bound:
tests/golden/shadow_binding_parent.json holds the output of tests/gen_shadow_binding.py, recorded from that earlier
library, and this file recomputes it.  The function touches no GPU, so a wrong offset, leading dimension, row0 or padding
in the one placement table of csrc/encoder.hip (which sgl_prepare_weights_dirty casts by as well) fails here, on the CPU.

The golden file is never re-recorded from the tree under test to make this pass.  A change that MEANS to move a shadow
regenerates it from the commit before that change (SGL_LIB_PATH=<that build's library> python tests/gen_shadow_binding.py)
and shows in the change itself which masters moved and why.
"""
import json

import pytest

import gen_shadow_binding as gen

CASES = [gen.case_name(cfg, head, mode) for cfg in gen.CONFIGS for head in (1, 0) for mode in gen.MODES]


@pytest.fixture(scope="module")
def got(pkg, hiplib):
    return gen.records(pkg)


@pytest.fixture(scope="module")
def want():
    with open(gen.OUT) as f:
        return json.load(f)


def test_the_same_cases_are_recorded(got, want):
    assert sorted(got) == sorted(want) == sorted(CASES)


@pytest.mark.parametrize("case", CASES)
def test_binding_matches_the_parent_library_field_for_field(got, want, case):
    g, w = got[case], want[case]
    assert g["return"] == w["return"], f"{case}: bound {g['return']} entries, the parent bound {w['return']}"
    assert sorted(g["masters"]) == sorted(w["masters"])
    moved = {m: (g["masters"][m], w["masters"][m]) for m in w["masters"] if g["masters"][m] != w["masters"][m]}
    assert not moved, f"{case}: {len(moved)} masters differ from the parent library (got, want): {list(moved.items())[:4]}"


@pytest.mark.parametrize("case", [c for c in CASES if c.endswith("/mxfp8")])
def test_mx_mode_binds_nothing(got, case):
    assert got[case]["return"] == 0
    assert all(rec is None for rec in got[case]["masters"].values()), f"{case}: an aux entry was written"


def test_bound_masters_are_the_matrices_and_fused_biases(got):
    """A reading aid for the golden file, and a check that it is not vacuous: per block q/k/v/o/fc1/fc2 weights with both
    copies and q/k/v/fc1 biases as fp32; the patch weight without a transposed copy; the head's in_proj_w from row D."""
    rec = got["hostile/head/bf16"]
    m = rec["masters"]
    bound = sorted(k for k, v in m.items() if v is not None)
    per_block = ["fc1_b", "fc1_w", "fc2_w", "k_b", "k_w", "o_w", "q_b", "q_w", "v_b", "v_w"]
    assert bound == sorted(["patch_w", "in_proj_w", "out_proj_w", "head_fc1_w", "head_fc2_w", "head_fc1_b"] +
                           [f"layers.{l}.{f}" for l in range(2) for f in per_block])
    assert rec["return"] == len(bound)
    assert m["patch_w"]["dst_t"] is None and m["patch_w"]["ld"] == 640 and m["patch_w"]["cols"] == 588
    assert m["in_proj_w"]["row0"] == 144 and m["in_proj_w"]["rows"] == 432 and m["in_proj_w"]["ld_t"] == 288
    assert m["layers.1.fc2_w"]["ld"] == 640 and m["layers.1.fc1_w"]["ld_t"] == 640      # Ip = 640 for I = 538
    assert got["hostile/nohead/bf16"]["return"] == len(bound) - 5
