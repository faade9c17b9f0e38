"""Ragged batches through the encoder: images of different sizes in one call (SiglipVisionModelHIP.forward_ragged,
sgl_forward_ragged).  The check that needs no tolerance: every image gets, bit for bit, what the existing per-image call
gives it alone, in all five compute modes.  The `hostile` config has so400m's head dimension (72 -> pad 80) and patch 14;
the images cover 1, 4, 9 (native), 21 (rectangular), 49 and 135 tokens (more than one 128-row query block), and one
size comes twice (the second copies the first one's position rows)."""
import ctypes as C
import dataclasses
import types

import pytest
import torch

import abi_harness as ah
from abi_harness import Arena, Session
from test_abi_contract_gpu import check_vs_oracle

pytestmark = pytest.mark.gpu

DEV = "cuda"
CFG = "hostile"
MODES = ["bf16", "fp16", "fp32", "bf16x3", "mxfp8"]
# (H, W) in pixels: 4, 1, 49, 21, 135 tokens, the native grid (9), and 28 x 28 again
SIZES = [(28, 28), (14, 14), (98, 98), (98, 42), (210, 126), (42, 42), (28, 28)]


def bits(t):
    return t.contiguous().view(torch.int32)


def images(pkg):
    return [pkg.weights.seeded_pixels(1, h, w, seed=31 + i)[0].to(DEV) for i, (h, w) in enumerate(SIZES)]


_CASES = {}


def case(pkg, mode):
    """(model, images, ragged output with all hidden states, per-image outputs), computed once per mode."""
    if mode not in _CASES:
        cfg = pkg.get_config(CFG)
        model = pkg.SiglipVisionModelHIP(cfg, compute_dtype=mode)
        model.load_state_dict(pkg.weights.seeded_state_dict(cfg, seed=19))
        model = model.to(DEV).requires_grad_(False)
        xs = images(pkg)
        with torch.no_grad():
            rag = model.forward_ragged(xs, output_hidden_states=True)
            single = [model(pixel_values=x[None], interpolate_pos_encoding=True, output_hidden_states=True) for x in xs]
        torch.cuda.synchronize()
        _CASES[mode] = (model, xs, rag, single)
    return _CASES[mode]


def assert_image_equal(rag, i, one, what):
    assert torch.equal(bits(rag.pooler_output[i]), bits(one.pooler_output[0])), f"{what}: pooler_output of image {i}"
    assert torch.equal(bits(rag.unpack(rag.last_hidden_state)[i]), bits(one.last_hidden_state[0])), \
        f"{what}: last_hidden_state of image {i}"
    assert len(rag.hidden_states) == len(one.hidden_states)
    for l, (a, b) in enumerate(zip(rag.hidden_states, one.hidden_states)):
        assert torch.equal(bits(rag.unpack(a)[i]), bits(b[0])), f"{what}: hidden_states[{l}] of image {i}"


@pytest.mark.parametrize("mode", MODES)
def test_every_image_equals_its_own_call_bitwise(pkg, hiplib, mode):
    model, xs, rag, single = case(pkg, mode)
    P, D = model.config.patch_size, model.config.hidden_size
    assert rag.grids == tuple((h // P, w // P) for h, w in SIZES)
    assert rag.cu_seqlens[-1] == sum(gh * gw for gh, gw in rag.grids) == rag.last_hidden_state.shape[0]
    assert rag.pooler_output.shape == (len(SIZES), D)
    assert rag.token_grid(rag.last_hidden_state, 4).shape == (15, 9, D)
    for i, one in enumerate(single):
        assert_image_equal(rag, i, one, mode)
    assert not torch.isnan(rag.last_hidden_state).any() and not torch.isnan(rag.pooler_output).any()


@pytest.mark.parametrize("mode", MODES)
def test_permuting_the_images_permutes_the_outputs(pkg, hiplib, mode):
    model, xs, rag, _ = case(pkg, mode)
    perm = [4, 0, 6, 2, 5, 1, 3]
    with torch.no_grad():
        out = model.forward_ragged([xs[j] for j in perm], output_hidden_states=True)
    for i, j in enumerate(perm):
        assert torch.equal(bits(out.pooler_output[i]), bits(rag.pooler_output[j]))
        assert torch.equal(bits(out.unpack(out.last_hidden_state)[i]), bits(rag.unpack(rag.last_hidden_state)[j]))
        for a, b in zip(out.hidden_states, rag.hidden_states):
            assert torch.equal(bits(out.unpack(a)[i]), bits(rag.unpack(b)[j]))


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_hidden_state_selection_and_a_model_without_the_head(pkg, hiplib, mode):
    model, xs, rag, _ = case(pkg, mode)
    L = model.config.num_hidden_layers
    with torch.no_grad():
        out = model.forward_ragged([x[None] for x in xs], hidden_state_ids=[-1, 0, 1])      # (1,3,H,W) inputs
        plain = model.forward_ragged(xs)
    assert plain.hidden_states is None
    assert torch.equal(bits(plain.last_hidden_state), bits(rag.last_hidden_state))
    assert len(out.hidden_states) == 3
    for got, l in zip(out.hidden_states, (L, 0, 1)):
        assert torch.equal(bits(got), bits(rag.hidden_states[l])), f"hidden_state_ids entry for slot {l}"
    cfg = dataclasses.replace(model.config, vision_use_head=False)
    bare = pkg.SiglipVisionModelHIP(cfg, compute_dtype=mode)
    bare.load_state_dict({k: v for k, v in pkg.weights.seeded_state_dict(model.config, seed=19).items()
                          if not k.startswith("head.")})
    bare = bare.to(DEV).requires_grad_(False)
    with torch.no_grad():
        o = bare.forward_ragged(xs, output_hidden_states=True)
    assert o.pooler_output is None
    assert torch.equal(bits(o.last_hidden_state), bits(rag.last_hidden_state))
    assert torch.equal(bits(o.hidden_states[L]), bits(rag.hidden_states[L]))


def test_fp32_against_the_oracle(pkg, oracle, hiplib):
    model, xs, rag, _ = case(pkg, "fp32")
    cfg = model.config
    sd = pkg.weights.seeded_state_dict(cfg, seed=19)
    for i, x in enumerate(xs):
        ref = oracle.vision_forward(x[None].cpu(), sd, cfg, True, True)
        want = {"last": ref["last_hidden_state"][0], "pooled": ref["pooler_output"][0]}
        got = {"last": rag.unpack(rag.last_hidden_state)[i], "pooled": rag.pooler_output[i]}
        for l, h in enumerate(ref["hidden_states"]):
            want[f"hs{l}"] = h[0]
            got[f"hs{l}"] = rag.unpack(rag.hidden_states[l])[i]
        check_vs_oracle(types.SimpleNamespace(out=want), got, {}, "fp32", f"ragged image {i} {SIZES[i]}")


@pytest.mark.parametrize("mode", ["bf16", "mxfp8"])
def test_encode_image_ragged_equals_encode_image(pkg, hiplib, mode):
    cfg = pkg.get_config(CFG)
    enc = pkg.OpenClipStyleEncoder(cfg, compute_dtype=mode)
    enc.visual.load_state_dict(pkg.weights.seeded_state_dict(cfg, seed=19))
    enc = enc.to(DEV).requires_grad_(False)
    xs = images(pkg)
    with torch.no_grad():
        f = enc.encode_image_ragged(xs)
        fn = enc.encode_image_ragged(xs, normalize=True)
        for i, x in enumerate(xs):
            if SIZES[i] == (42, 42):
                one = enc.encode_image(x[None])
            else:       # encode_image itself takes the native size only
                one = enc.visual(pixel_values=x[None], interpolate_pos_encoding=True).pooler_output
            assert torch.equal(bits(f[i]), bits(one[0])), f"image {i}"
    assert torch.equal(bits(fn), bits(f / f.norm(dim=-1, keepdim=True)))


def test_a_head_trains_on_a_frozen_backbone(pkg, hiplib):
    model, xs, _, _ = case(pkg, "bf16")
    D = model.config.hidden_size
    grads = []
    for route in ("ragged", "per image"):
        torch.manual_seed(3)
        head = torch.nn.Linear(D, 2).to(DEV)
        assert torch.is_grad_enabled()
        if route == "ragged":
            feats = model.forward_ragged(xs).pooler_output
        else:
            feats = torch.cat([model(pixel_values=x[None], interpolate_pos_encoding=True).pooler_output for x in xs])
        head(feats).square().sum().backward()
        grads.append((head.weight.grad.clone(), head.bias.grad.clone()))
    assert torch.equal(bits(grads[0][0]), bits(grads[1][0])) and torch.equal(bits(grads[0][1]), bits(grads[1][1]))
    assert float(grads[0][0].abs().max()) > 0


# ---- through the C ABI, with guarded and poisoned arenas ---------------------------------------------------------
def ragged_abi_call(ses, shadow, operand, grids, fill):
    """sgl_forward_ragged with every arena filled with `fill` first.  Returns (status, outputs dict, arenas)."""
    lib, L, D = ses.lib, ses.Lyr, ses.D
    S = len(grids)
    T = sum(gh * gw for gh, gw in grids)
    flat = (C.c_int * (2 * S))(*[v for g in grids for v in g])
    n = C.c_size_t()
    assert lib.sgl_query_sizes_ragged(ses.ctx, flat, S, C.byref(n)) == ah.OK
    ws = Arena(n.value, fill)
    hs = [Arena(T * D * 4, fill) for _ in range(L + 1)]
    last, pooled = Arena(T * D * 4, fill), Arena(S * D * 4, fill)
    table = (C.c_void_p * (L + 1))(*[a.ptr for a in hs])
    st = lib.sgl_forward_ragged(ses.ctx, C.byref(ses.w), shadow.ptr, operand.data_ptr(), flat, S, table, last.ptr,
                                pooled.ptr if ses.use_head else None, ws.ptr, ws.nbytes, ah.stream())
    torch.cuda.synchronize()
    out = {"last": last.f32(T, D).clone(), "pooled": pooled.f32(S, D).clone()}
    for l, a in enumerate(hs):
        out[f"hs{l}"] = a.f32(T, D).clone()
    arenas = [("ws", ws), ("last", last), ("pooled", pooled)] + [(f"hs{l}", a) for l, a in enumerate(hs)]
    return st, out, arenas


@pytest.mark.parametrize("mode", MODES)
def test_c_abi_writes_only_its_arenas_and_ignores_what_ws_held(pkg, hiplib, mode):
    with Session(pkg, hiplib, CFG, mode, 0, seed=19) as ses:
        shadow = ses.new_shadow(0xFF)
        assert ses.prepare(shadow, full=True) == ah.OK
        P = ses.P
        grids = [(h // P, w // P) for h, w in SIZES]
        operand = torch.cat([ses.patch_operand(x[None].contiguous(), 1, h, w) for x, (h, w) in zip(images(pkg), SIZES)])
        before = operand.clone()
        results = []
        for fill in (0xFF, 0x00):          # 0xFF bytes read as NaN in every operand type
            st, out, arenas = ragged_abi_call(ses, shadow, operand, grids, fill)
            assert st == ah.OK
            ah.assert_guards(arenas + [("shadow", shadow)], f"sgl_forward_ragged {mode} fill {fill:#x}")
            for k, v in out.items():
                assert not torch.isnan(v).any(), f"{mode} fill {fill:#x}: {k} holds a NaN"
            results.append(out)
        for k in results[0]:
            assert torch.equal(bits(results[0][k]), bits(results[1][k])), f"{mode}: {k} depends on what ws held before"
        assert torch.equal(operand.view(torch.uint8), before.view(torch.uint8)), "the patch operand was written"
        # the package's call is this one
        _, _, rag, _ = case(pkg, mode)
        assert torch.equal(bits(results[0]["last"]), bits(rag.last_hidden_state))
        assert torch.equal(bits(results[0]["pooled"]), bits(rag.pooler_output))
