"""CPU (no GPU): the state a SiglipVisionModelHIP keeps between calls (encoder_state.py).

* C contexts die exactly once, with the module that created them: a shallow copy and an unpickled copy own theirs;
* parameter table, shadow units, gradient chunk layouts and slot plans equal what the commit before the split into
  surfaces / ops / state owners produced (tests/golden/encoder_plans_parent.json, tests/gen_encoder_plans.py);
* the pointer the weights struct holds for a table entry is that of the parameter at the entry's HF path.
"""
import copy
import gc
import json
import pickle

import pytest

import gen_encoder_plans as gen


def test_contexts_die_once_with_the_module_that_made_them(pkg, hiplib, monkeypatch):
    destroyed = []
    really_destroy = hiplib.sgl_destroy
    monkeypatch.setattr(hiplib, "sgl_destroy", destroyed.append)       # nothing recorded here is ever called into again
    try:
        m = pkg.SiglipVisionModelHIP(pkg.get_config("tiny"), "bf16")
        sizes = m._contexts.sizes(2, 32, 32, True), m._contexts.sizes(2, 32, 32, True, True)   # creates both contexts
        mine = [m._contexts.get(False), m._contexts.get(True)]
        assert all(mine) and mine[0] != mine[1]

        c = copy.copy(m)
        del c
        gc.collect()
        assert destroyed == [], "deleting an unused shallow copy destroyed a context of the original"
        u = pickle.loads(pickle.dumps(m))
        del u
        gc.collect()
        assert destroyed == [], "deleting an unused unpickled copy destroyed a context of the original"

        c, u = copy.copy(m), pickle.loads(pickle.dumps(m))
        assert len({m._handle, c._handle, u._handle}) == 3
        assert all(a is b for a, b in zip(c._table.params(), m._table.params()))       # same parameters ...
        theirs = []
        for other in (c, u):                                                            # ... contexts of their own
            assert (other._contexts.sizes(2, 32, 32, True), other._contexts.sizes(2, 32, 32, True, True)) == sizes
            theirs += [other._contexts.get(False), other._contexts.get(True)]
        assert len(set(theirs + mine)) == 6
        assert [m._contexts.get(False), m._contexts.get(True)] == mine
        del c, u, other
        gc.collect()
        assert sorted(destroyed) == sorted(theirs)
        del m
        gc.collect()
        assert sorted(destroyed[4:]) == sorted(mine), "each context of the module exactly once"
    finally:
        monkeypatch.undo()
        for ctx in destroyed:
            really_destroy(ctx)


@pytest.fixture(scope="module")
def parent_plans():
    with open(gen.OUT) as f:
        return json.load(f)


def test_plan_record_covers_every_model(parent_plans):
    assert sorted(parent_plans) == sorted(f"{n}/{h}" for n in gen.SMALL + gen.LARGE for h in ("head", "nohead"))


@pytest.mark.parametrize("use_head", [True, False], ids=["head", "nohead"])
@pytest.mark.parametrize("name", gen.SMALL + gen.LARGE)
def test_plans_equal_the_parent_commits(pkg, parent_plans, name, use_head):
    want = parent_plans[f"{name}/{'head' if use_head else 'nohead'}"]
    got = gen.record(pkg, gen.Current, name, use_head, name in gen.SMALL)
    L = pkg.get_config(name).num_hidden_layers
    n_patterns = 4 + L + 16 + 1              # all, none, head, emb; frozen below 1..L; each field of block 1; q_w of block 0
    assert len(want["layouts"]) == n_patterns * len(gen.MAX_BUCKETS) and len(want["slots"]) == 10
    if name in gen.SMALL:
        assert isinstance(want["table"], list) and all(isinstance(want["layouts"][k], dict) for k in gen.FULL_LAYOUTS)
    assert got["table"] == want["table"]
    assert got["units"] == want["units"]
    assert got["slots"] == want["slots"]
    assert set(got["layouts"]) == set(want["layouts"])
    moved = [k for k in want["layouts"] if got["layouts"][k] != want["layouts"][k]]
    assert not moved, f"{len(moved)} chunk layouts moved, e.g. {moved[0]}"


def test_weights_struct_points_at_the_parameter_of_each_hf_path(pkg):
    m = pkg.SiglipVisionModelHIP(pkg.get_config("tiny"), "bf16")
    assert m.use_head
    params = m._table.params()
    w, layers, _ = m._shadows._weights_struct(params)
    named = dict(m.named_parameters())
    assert len(m._table.entries) == len(named) == len({p.data_ptr() for p in params})
    for e in m._table.entries:
        holder = w if e.block is None else layers[e.block]
        assert getattr(holder, e.field) == named[e.path].data_ptr() == m.get_parameter(e.path).data_ptr(), e
        assert "vision_model." + e.path in m.state_dict()
    # the spec itself, against attribute accesses written out by hand (q / k / v have equal shapes: only this tells them apart)
    blk = m.encoder.layers[1]
    for got, param in [(layers[1].q_w, blk.self_attn.q_proj.weight), (layers[1].k_w, blk.self_attn.k_proj.weight),
                       (layers[1].v_w, blk.self_attn.v_proj.weight), (layers[1].q_b, blk.self_attn.q_proj.bias),
                       (layers[1].k_b, blk.self_attn.k_proj.bias), (layers[1].v_b, blk.self_attn.v_proj.bias),
                       (layers[1].o_w, blk.self_attn.out_proj.weight), (layers[1].ln1_w, blk.layer_norm1.weight),
                       (layers[1].ln2_b, blk.layer_norm2.bias), (layers[1].fc1_w, blk.mlp.fc1.weight),
                       (w.layers[2].fc2_b, m.encoder.layers[2].mlp.fc2.bias),
                       (w.patch_w, m.embeddings.patch_embedding.weight), (w.patch_b, m.embeddings.patch_embedding.bias),
                       (w.pos, m.embeddings.position_embedding.weight), (w.post_ln_w, m.post_layernorm.weight),
                       (w.probe, m.head.probe), (w.in_proj_w, m.head.attention.in_proj_weight),
                       (w.in_proj_b, m.head.attention.in_proj_bias), (w.out_proj_w, m.head.attention.out_proj.weight),
                       (w.head_ln_b, m.head.layernorm.bias), (w.head_fc1_w, m.head.mlp.fc1.weight),
                       (w.head_fc2_b, m.head.mlp.fc2.bias)]:
        assert got == param.data_ptr()
