"""GPU: the encoder C ABI (include/siglip_hip.h) called directly, the way INTEGRATION.md section 2 binds it, on guarded and
poisoned arenas (tests/abi_harness.py).  The single kernels are held to fp64 bounds in tests/test_kernel_edges_gpu.py;
this module tests what sits between them and the caller: the arena layout, the pad regions, the entry-point families and
the gradient-destination contract (NULL = frozen, accumulate, need_dx, optional d_* inputs).

Entry point -> a test that calls it
    sgl_create_ex / sgl_destroy / sgl_query_sizes   every test (abi_harness.Session); sgl_create: tests/test_abi_host.py
    sgl_last_hip_error / sgl_status_string / sgl_abi_version   test_status_helpers (and tests/test_abi_host.py)
    sgl_prepare_weights, sgl_prepare_weights_dirty  test_prepare_weights_equals_dirty_all, test_partial_shadow_refresh
    sgl_forward, sgl_forward_ex, sgl_forward_slots  test_forward_entry_points_bitwise, test_forward_two_slot_ping_pong
    sgl_backward, sgl_backward_begin, sgl_backward_layer, sgl_backward_embed,
    sgl_backward_begin_p, sgl_backward_layer_p      test_backward_entry_points_bitwise
Argument errors (every early return) are in tests/test_abi_contract_host.py and are not repeated here.

Numbers.  Three kinds of bar only: bitwise (torch.equal; the kernels are deterministic and the families differ in pointer
arithmetic alone), the project's bars from tests/test_encoder_gpu.py::test_forward_backward_vs_hf_golden (activations 2e-5
abs in fp32, gradients 1e-7 + 6e-5 * max|ref| per tensor, bf16x3 six times both, k_proj.bias against the q_proj.weight
scale), and 2^-22 * (|G0| + |g|) for one extra fp32 addition per partial when accumulating.  Every test prints its worst
error / bound.
"""
import pytest
import torch

import abi_harness as ah
from abi_harness import Arena, Grads, Reference, Run, Session

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS_ACC = 2.0 ** -22
IMAGES = {   # native, square interpolated, rectangular, non-divisible rectangular (trailing pixels beyond the last patch)
    "tiny": {"native": (32, 32), "square": (48, 48), "rect": (32, 48), "nondiv": (37, 53)},
    "hostile": {"native": (42, 42), "square": (56, 56), "rect": (42, 70), "nondiv": (101, 59)},
    "so400m-1layer": {"native": (384, 384)},
}


def taps_of(L):
    return tuple(sorted({min(1, L), L}))      # one inner tap and hidden_states[L] (d_tap_last)


def device_upstream(ses, B, H, W, terms=(1, 1, 1), taps=None):
    """(d_last, d_pooled, d_taps): the constant gradients of oracle.probe_loss (abi_harness.upstream), None where absent."""
    _, _, N, _ = ses.geometry(B, H, W)
    L = ses.Lyr
    up = ah.upstream(B, N, ses.D, L, taps_of(L) if taps is None else taps)
    d_pooled = up["pooled"].to(DEV) if (terms[0] and ses.use_head) else None
    d_last = up["last"].to(DEV).contiguous() if terms[1] else None
    d_taps = [up["taps"][l].to(DEV).contiguous() if l in up["taps"] else None for l in range(L + 1)] if terms[2] else None
    return d_last, d_pooled, d_taps


def layout_pixels(ses, px, B, H, W, channels_last):
    if channels_last == 1:
        return px.permute(0, 2, 3, 1).contiguous()      # NHWC storage
    if channels_last == 2:
        return ses.patch_operand(px, B, H, W)
    return px


def train_once(ses, B, H, W, *, fill=0x00, kind="contiguous", bwd=None, ex=False, ftb_fwd=0, ftb=0, temb=1, present=None,
               adjacent=True, accumulate=0, prior=None, terms=(1, 1, 1), channels_last=0, pixel_seed=1, passes=1,
               grad_fill=None, what=""):
    """prepare -> training forward -> (workspace re-poisoned) -> backward, everything in arenas filled `fill`.
    Returns outputs, gradients (GPU clones), and whether `pooled` was left untouched."""
    shadow = ses.new_shadow(fill)
    assert ses.prepare(shadow, full=True) == ah.OK
    run = Run(ses, B, H, W, True, fill, "slots" if kind == "slots" else "contiguous")
    px = layout_pixels(ses, ses.pixels(B, H, W, pixel_seed), B, H, W, channels_last)
    st = ses.forward(run, shadow, px, kind="slots" if kind == "slots" else "contiguous", ex=ex or ftb_fwd != 0,
                     channels_last=channels_last, first_trainable=ftb_fwd)
    assert st == ah.OK, f"{what}: forward status {st}"
    out = run.outputs(pooled=bool(ses.use_head))
    pooled_untouched = run.pooled.untouched()
    d_last, d_pooled, d_taps = device_upstream(ses, B, H, W, terms)
    G = Grads(ses, present, adjacent, accumulate, prior, fill if grad_fill is None else grad_fill)
    for _ in range(passes):
        # nothing in ws has to survive from the forward to sgl_backward_begin, on either kind of context
        st = ses.backward(run, shadow, G, kind=bwd or kind, d_last=d_last, d_pooled=d_pooled, d_taps=d_taps,
                          first_trainable=ftb, train_embeddings=temb, poison_ws=fill)
        assert st == ah.OK, f"{what}: backward status {st}"
    torch.cuda.synchronize()
    ah.assert_guards(run.arenas() + G.arenas() + [("shadow", shadow)], what)
    return {"out": out, "grads": G.gpu(), "pooled_untouched": pooled_untouched, "hs_after": run.outputs(bool(ses.use_head))}


def infer_once(ses, B, H, W, *, fill=0x00, kind="contiguous", n_slots=None, channels_last=0, pooled=True, pixel_seed=1,
               what=""):
    shadow = ses.new_shadow(fill)
    assert ses.prepare(shadow, full=True) == ah.OK
    run = Run(ses, B, H, W, False, fill, kind, n_slots)
    px = layout_pixels(ses, ses.pixels(B, H, W, pixel_seed), B, H, W, channels_last)
    st = ses.forward(run, shadow, px, kind=kind, channels_last=channels_last, pooled=pooled)
    assert st == ah.OK, f"{what}: forward status {st}"
    torch.cuda.synchronize()
    ah.assert_guards(run.arenas() + [("shadow", shadow)], what)
    return run


def assert_same(a, b, what, keys=None):
    for k in (keys if keys is not None else a.keys()):
        assert k in b, f"{what}: `{k}` missing"
        assert torch.equal(a[k], b[k]), f"{what}: `{k}` differs (max |diff| {(a[k] - b[k]).abs().max().item():.3e})"


def assert_finite(d, what):
    for k, v in d.items():
        assert bool(torch.isfinite(v).all()), f"{what}: `{k}` holds a NaN / inf (computed from a byte nobody wrote?)"


def package_model(pkg, ses, recompute=False):
    model = pkg.SiglipVisionModelHIP(ses.cfg, compute_dtype=ses.mode, recompute=recompute)
    model.load_state_dict(pkg.weights.seeded_state_dict(ses.cfg, seed=ses.seed))
    return model.to(DEV)


def package_outputs(out, M, D):
    o = {"last": out.last_hidden_state.detach().reshape(M, D)}
    if out.pooler_output is not None:
        o["pooled"] = out.pooler_output.detach()
    for l, h in enumerate(out.hidden_states):
        o[f"hs{l}"] = h.detach().reshape(M, D)
    return o


def test_status_helpers(pkg, hiplib):
    with Session(pkg, hiplib, "tiny", "bf16") as ses:
        assert hiplib.sgl_last_hip_error(ses.ctx) == 0
        assert hiplib.sgl_abi_version() == 3 and hiplib.sgl_status_string(ah.ERR_NULL) == b"null pointer"
        run = infer_once(ses, 1, 32, 32)
        assert bool(torch.isfinite(run.pooled.f32(1, ses.D)).all()) and hiplib.sgl_last_hip_error(ses.ctx) == 0


# =====================================================================================================================
# a. every entry-point family gives the same bits
# =====================================================================================================================
@pytest.mark.parametrize("mode", ah.TRAIN_MODES + ["mxfp8"])
@pytest.mark.parametrize("cfg_name,HW", [("tiny", (32, 32)), ("hostile", (56, 42))])
def test_forward_entry_points_bitwise(pkg, hiplib, cfg_name, HW, mode):
    """sgl_forward (hs_slots = L+1) == sgl_forward_ex(first_trainable_block = 0) == sgl_forward_slots == the package."""
    B, (H, W) = 2, HW
    train = mode != "mxfp8"
    with Session(pkg, hiplib, cfg_name, mode, seed=3) as ses:
        shadow = ses.new_shadow()
        assert ses.prepare(shadow, full=True) == ah.OK
        px = ses.pixels(B, H, W, 5)
        outs = {}
        for label, kind, ex in (("sgl_forward", "contiguous", False), ("sgl_forward_ex", "contiguous", True),
                                ("sgl_forward_slots", "slots", False)):
            run = Run(ses, B, H, W, train, 0x00, kind)
            assert ses.forward(run, shadow, px, kind=kind, ex=ex) == ah.OK, label
            outs[label] = run.outputs()
            ah.assert_guards(run.arenas(), label)
        model = package_model(pkg, ses)
        M = B * (H // ses.P) * (W // ses.P)
        with torch.set_grad_enabled(train):
            o = model(pixel_values=px, output_hidden_states=True, interpolate_pos_encoding=True)
        outs["package"] = package_outputs(o, M, ses.D)
        assert len(outs["sgl_forward"]) == ses.Lyr + 3
        for label in ("sgl_forward_ex", "sgl_forward_slots", "package"):
            assert_same(outs["sgl_forward"], outs[label], f"sgl_forward vs {label} [{cfg_name}/{mode}]")
        assert_finite(outs["sgl_forward"], "sgl_forward")


@pytest.mark.parametrize("mode", ["fp32", "bf16x3", "bf16", "fp16", "mxfp8"])
@pytest.mark.parametrize("cfg_name", ["tiny", "hostile"])      # L = 3 (odd) and L = 2 (even)
def test_forward_two_slot_ping_pong(pkg, hiplib, cfg_name, mode):
    """Inference sgl_forward with hs_slots = 2: pooled and last equal the L+1 run; slot L % 2 holds hidden_states[L] and
    slot (L-1) % 2 holds hidden_states[L-1]."""
    H, W = IMAGES[cfg_name]["rect"]
    with Session(pkg, hiplib, cfg_name, mode, seed=4) as ses:
        L = ses.Lyr
        full = infer_once(ses, 2, H, W, what="L+1 slots")
        two = infer_once(ses, 2, H, W, n_slots=2, what="2 slots")
        assert torch.equal(full.pooled.payload, two.pooled.payload) and torch.equal(full.last.payload, two.last.payload)
        assert torch.equal(two.slot(L % 2), full.hidden(L)), "slot L % 2 is not hidden_states[L]"
        assert torch.equal(two.slot((L - 1) % 2), full.hidden(L - 1)), "slot (L-1) % 2 is not hidden_states[L-1]"
        assert bool(torch.isfinite(full.pooled.f32(2, ses.D)).all())


@pytest.mark.parametrize("mode", ["fp32", "bf16x3", "bf16", "fp16", "mxfp8"])
@pytest.mark.parametrize("cfg_name", ["tiny", "hostile"])
def test_prepare_weights_equals_dirty_all(pkg, hiplib, cfg_name, mode):
    with Session(pkg, hiplib, cfg_name, mode, seed=2) as ses:
        a, b = ses.new_shadow(0xFF), ses.new_shadow(0xFF)
        assert ses.prepare(a, full=True) == ah.OK
        assert ses.prepare(b, dirty=None, globals_dirty=1) == ah.OK
        assert torch.equal(a.payload, b.payload)
        assert not a.untouched() and a.guards_intact() and b.guards_intact()


def present_for(ses, ftb, temb):
    """Destinations sgl_backward(first_trainable_block, train_embeddings) never writes are NULL (as the package passes)."""
    stop = 0 if temb else ftb
    pres = {}
    if not temb:
        for n in ("patch_w", "patch_b", "pos"):
            pres[ah.GLOBAL_NAMES[n]] = False
    for l in range(stop):
        for f in ah.LAYER_NAMES:
            pres[ah.layer_name(l, f)] = False
    return pres


@pytest.mark.parametrize("recompute", [0, 1])
@pytest.mark.parametrize("mode", ah.TRAIN_MODES)
@pytest.mark.parametrize("cfg_name,HW", [("tiny", (32, 32)), ("hostile", (56, 42))])
def test_backward_entry_points_bitwise(pkg, hiplib, cfg_name, HW, mode, recompute):
    """sgl_backward == begin -> layer (L-1..stop) -> embed == the _p loop == the package's .grad, for
    (first_trainable_block, train_embeddings) in {(0,1), (0,0), (1,0), (L,0)} and with d_taps given / NULL."""
    B, (H, W) = 2, HW
    with Session(pkg, hiplib, cfg_name, mode, recompute, seed=6) as ses:
        L = ses.Lyr
        shadow = ses.new_shadow()
        assert ses.prepare(shadow, full=True) == ah.OK
        px = ses.pixels(B, H, W, 7)
        run_c, run_s = Run(ses, B, H, W, True, 0x00, "contiguous"), Run(ses, B, H, W, True, 0x00, "slots")
        assert ses.forward(run_c, shadow, px, kind="contiguous") == ah.OK
        assert ses.forward(run_s, shadow, px, kind="slots") == ah.OK
        model = package_model(pkg, ses, recompute=bool(recompute))
        named = dict(model.named_parameters())
        up = ah.upstream(B, run_c.N, ses.D, L, taps_of(L))
        for ftb, temb in ((0, 1), (0, 0), (1, 0), (L, 0)):
            pres = present_for(ses, ftb, temb)
            for with_taps in (True, False):
                what = f"{cfg_name}/{mode}/rc{recompute} ftb={ftb} emb={temb} taps={with_taps}"
                d_last, d_pooled, d_taps = device_upstream(ses, B, H, W, (1, 1, 1 if with_taps else 0))
                res = {}
                for label, run, kind in (("sgl_backward", run_c, "contiguous"), ("begin/layer/embed", run_c, "steps"),
                                         ("begin_p/layer_p/embed", run_s, "slots")):
                    G = Grads(ses, pres)
                    st = ses.backward(run, shadow, G, kind=kind, d_last=d_last, d_pooled=d_pooled, d_taps=d_taps,
                                      first_trainable=ftb, train_embeddings=temb, poison_ws=0xFF)
                    assert st == ah.OK, (what, label, st)
                    res[label] = G.gpu()
                    ah.assert_guards(G.arenas() + run.arenas(), f"{what} {label}")
                assert_finite(res["sgl_backward"], what)
                for label in ("begin/layer/embed", "begin_p/layer_p/embed"):
                    assert_same(res["sgl_backward"], res[label], f"{what}: sgl_backward vs {label}")
                # the package on the same weights, pixels and upstream gradients
                for n, p in named.items():
                    p.requires_grad_(pres.get(n, True))
                    p.grad = None
                o = model(pixel_values=px, output_hidden_states=True, interpolate_pos_encoding=True)
                loss = (o.pooler_output * up["pooled"].to(DEV)).sum() + (o.last_hidden_state * up["last"].to(DEV)).sum()
                if with_taps:
                    for i, u in up["taps"].items():
                        loss = loss + (o.hidden_states[i] * u.to(DEV)).sum()
                loss.backward()
                got = {n: p.grad.detach() for n, p in named.items() if pres.get(n, True)}
                assert set(got) == set(res["sgl_backward"])
                assert_same(res["sgl_backward"], got, f"{what}: sgl_backward vs package")


@pytest.mark.parametrize("recompute", [0, 1])
@pytest.mark.parametrize("mode", ah.TRAIN_MODES)
@pytest.mark.parametrize("cfg_name", ["tiny", "hostile"])
def test_forward_ex_frozen_prefix_gradients(pkg, hiplib, cfg_name, mode, recompute):
    """sgl_forward_ex(first_trainable_block = k) + a backward stopping at k == the k = 0 forward's gradients for blocks >= k:
    the GELU pre-activations the frozen blocks did not save are never read (saved is 0xFF-filled here)."""
    H, W = IMAGES[cfg_name]["square"]
    with Session(pkg, hiplib, cfg_name, mode, recompute, seed=8) as ses:
        for k in range(1, ses.Lyr + 1):
            pres = present_for(ses, k, 0)
            a = train_once(ses, 2, H, W, fill=0xFF, ftb_fwd=0, ftb=k, temb=0, present=pres, what="k=0 forward")
            b = train_once(ses, 2, H, W, fill=0xFF, ftb_fwd=k, ftb=k, temb=0, present=pres, what=f"k={k} forward")
            assert_same(a["out"], b["out"], f"forward_ex k={k} outputs")
            assert_same(a["grads"], b["grads"], f"forward_ex k={k} gradients")
            assert_finite(b["grads"], f"forward_ex k={k}")


@pytest.mark.parametrize("mode", ah.TRAIN_MODES + ["mxfp8"])
def test_channels_last_variants_bitwise(pkg, hiplib, mode):
    """channels_last 0 (NCHW), 1 (NHWC storage) and 2 (the ready patch operand, sgl_op_im2col's output) give the same bits."""
    H, W = IMAGES["hostile"]["nondiv"]
    with Session(pkg, hiplib, "hostile", mode, seed=9) as ses:
        res = []
        for cl in (0, 1, 2):
            if mode == "mxfp8":
                run = infer_once(ses, 2, H, W, fill=0xFF, channels_last=cl, what=f"channels_last={cl}")
                res.append({"out": run.outputs(), "grads": {}})
            else:
                res.append(train_once(ses, 2, H, W, fill=0xFF, channels_last=cl, what=f"channels_last={cl}"))
        for cl in (1, 2):
            assert_same(res[0]["out"], res[cl]["out"], f"channels_last 0 vs {cl} outputs")
            assert_same(res[0]["grads"], res[cl]["grads"], f"channels_last 0 vs {cl} gradients")
        assert_finite(res[0]["out"], mode)
        assert_finite(res[0]["grads"], mode)


# =====================================================================================================================
# b. the arena contract
# =====================================================================================================================
T, I_ = True, False
ARENA_CASES = [
    # config, mode, policy, train, use_head, B, image
    # hostile: every (mode, policy, train / inference), B = 3, non-divisible rectangular image (7 x 4 grid)
    ("hostile", "fp32", 0, T, 1, 3, "nondiv"), ("hostile", "fp32", 1, T, 1, 3, "nondiv"),
    ("hostile", "fp32", 0, I_, 1, 3, "nondiv"), ("hostile", "fp32", 1, I_, 1, 3, "nondiv"),
    ("hostile", "bf16x3", 0, T, 1, 3, "nondiv"), ("hostile", "bf16x3", 1, T, 1, 3, "nondiv"),
    ("hostile", "bf16x3", 0, I_, 1, 3, "nondiv"), ("hostile", "bf16x3", 1, I_, 1, 3, "nondiv"),
    ("hostile", "bf16", 0, T, 1, 3, "nondiv"), ("hostile", "bf16", 1, T, 1, 3, "nondiv"),
    ("hostile", "bf16", 0, I_, 1, 3, "nondiv"), ("hostile", "bf16", 1, I_, 1, 3, "nondiv"),
    ("hostile", "fp16", 0, T, 1, 3, "nondiv"), ("hostile", "fp16", 1, T, 1, 3, "nondiv"),
    ("hostile", "fp16", 0, I_, 1, 3, "nondiv"), ("hostile", "fp16", 1, I_, 1, 3, "nondiv"),
    ("hostile", "mxfp8", 0, I_, 1, 3, "nondiv"),
    # the remaining axes (use_head 0, B = 1, native / square / rectangular) in bf16 and in bf16x3, both policies
    ("hostile", "bf16", 0, T, 0, 1, "native"), ("hostile", "bf16", 1, T, 1, 1, "square"),
    ("hostile", "bf16", 1, T, 0, 3, "rect"), ("hostile", "bf16", 0, I_, 0, 1, "rect"),
    ("hostile", "bf16x3", 1, T, 0, 1, "native"), ("hostile", "bf16x3", 0, T, 1, 1, "square"),
    ("hostile", "bf16x3", 0, T, 0, 3, "rect"), ("hostile", "bf16x3", 0, I_, 0, 1, "rect"),
    ("hostile", "mxfp8", 0, I_, 0, 1, "native"),
    # pad-free layout
    ("tiny", "bf16", 0, T, 1, 3, "native"), ("tiny", "fp16", 1, T, 1, 1, "nondiv"), ("tiny", "mxfp8", 0, I_, 1, 3, "rect"),
    # production layout (head_dim 72 -> 80, I 4304 -> 4352, 588 -> 640)
    ("so400m-1layer", "bf16", 0, T, 1, 1, "native"), ("so400m-1layer", "fp16", 1, T, 1, 1, "native"),
    ("so400m-1layer", "mxfp8", 0, I_, 1, 1, "native"),
]


@pytest.mark.parametrize("cfg_name,mode,recompute,train,use_head,B,image", ARENA_CASES,
                         ids=[f"{c}-{m}-rc{r}-{'train' if t else 'infer'}-head{h}-B{b}-{im}"
                              for c, m, r, t, h, b, im in ARENA_CASES])
def test_arena_contract_zero_and_poison_fill(pkg, hiplib, cfg_name, mode, recompute, train, use_head, B, image):
    """Sizes exactly as sgl_query_sizes reports.  One run with every arena, slot, output and gradient destination filled
    0x00 and one filled 0xFF (the shadow before sgl_prepare_weights, the workspace again before sgl_backward_begin): outputs
    and gradients are bit-identical and finite (a difference means a kernel read bytes nobody wrote), every guard band is
    intact, and `pooled` passed with use_head = 0 comes back untouched."""
    H, W = IMAGES[cfg_name][image]
    res = []
    with Session(pkg, hiplib, cfg_name, mode, recompute, use_head, seed=11) as ses:
        for fill in (0x00, 0xFF):
            what = f"fill {fill:#04x}"
            if train:
                r = train_once(ses, B, H, W, fill=fill, what=what)
                assert_same(r["out"], r["hs_after"], what + ": the backward changed a forward output")
            else:
                run = infer_once(ses, B, H, W, fill=fill, n_slots=2, what=what)
                r = {"out": run.outputs(pooled=bool(use_head)), "grads": {}, "pooled_untouched": run.pooled.untouched()}
                r["out"]["slot0"], r["out"]["slot1"] = run.slot(0).clone(), run.slot(1).clone()
            if not use_head:
                assert r["pooled_untouched"], what + ": pooled was written although use_head == 0"
            assert_finite(r["out"], what)
            assert_finite(r["grads"], what)
            res.append(r)
    assert_same(res[0]["out"], res[1]["out"], "0x00 vs 0xFF outputs")
    assert_same(res[0]["grads"], res[1]["grads"], "0x00 vs 0xFF gradients")
    if train:
        assert len(res[0]["grads"]) == len(pkg.weights.param_shapes(ah.make_config(pkg, cfg_name, use_head)))


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("cfg_name", ["tiny", "hostile"])
def test_pooled_null_leaves_other_outputs_equal(pkg, hiplib, cfg_name, train):
    H, W = IMAGES[cfg_name]["rect"]
    with Session(pkg, hiplib, cfg_name, "bf16", seed=12) as ses:
        shadow = ses.new_shadow(0xFF)
        assert ses.prepare(shadow, full=True) == ah.OK
        px = ses.pixels(2, H, W, 3)
        outs = []
        for pooled in (True, False):
            run = Run(ses, 2, H, W, train, 0xFF)
            assert ses.forward(run, shadow, px, pooled=pooled) == ah.OK
            torch.cuda.synchronize()
            ah.assert_guards(run.arenas(), f"pooled={pooled}")
            outs.append(run.outputs(pooled=False))
            assert run.pooled.untouched() == (not pooled)
        assert_same(outs[0], outs[1], "pooled = NULL")
        assert_finite(outs[1], "pooled = NULL")


# =====================================================================================================================
# c. gradient destinations
# =====================================================================================================================
def seeded_prior(pkg, shapes, scale_of, seed):
    """G0 = scale * uniform(-1, 1) per destination, scale = the gradient's own magnitude."""
    return {n: pkg.weights.seeded_tensor("g0." + n, shp, max(scale_of(n), 1e-30), seed) for n, shp in shapes.items()}


@pytest.mark.parametrize("recompute", [0, 1])
@pytest.mark.parametrize("mode", ["fp32", "bf16x3"])
@pytest.mark.parametrize("cfg_name,image", [("hostile", "native"), ("hostile", "nondiv"), ("tiny", "native"),
                                            ("tiny", "rect")])
def test_accumulate_vs_oracle(pkg, oracle, hiplib, cfg_name, image, mode, recompute):
    """accumulate = 1 onto G0: result - G0 meets the project's gradient bar widened by 2^-22 * (|G0| + |ref|); a second
    pass (micro-batch 2) gives G0 + 2 g; k_proj.bias comes back as G0 bit for bit.  Covers the native and the interpolated
    position gradient and both writers of in_proj_weight / in_proj_bias."""
    B, (H, W) = 2, IMAGES[cfg_name][image]
    with Session(pkg, hiplib, cfg_name, mode, recompute, seed=13) as ses:
        ref = Reference.get(pkg, oracle, cfg_name, 13, B, H, W, 1, taps_of(ses.Lyr))
        shapes = pkg.weights.param_shapes(ses.cfg)
        qb = "encoder.layers.0.self_attn.q_proj.bias"

        def scale(n):
            return float(ref.grads[qb if n.endswith("k_proj.bias") else n].abs().max())
        G0 = seeded_prior(pkg, shapes, scale, 31)
        worst = {}
        for passes in (1, 2):
            r = train_once(ses, B, H, W, fill=0xFF, accumulate=1, prior=G0, passes=passes, what=f"accumulate x{passes}")
            for n, got in r["grads"].items():
                g0, rg = G0[n], ref.grads[n]
                if n.endswith("k_proj.bias"):
                    assert torch.equal(got.cpu(), g0), f"{n}: accumulate = 1 must leave G0 untouched (exact zero gradient)"
                    continue
                err = (got.cpu().double() - g0.double() - passes * rg.double()).abs()
                # `passes` results each within the bar, one extra fp32 addition at magnitude |G0| + passes |ref| per pass
                bound = passes * ref.bar(n, mode) + passes * EPS_ACC * (g0.abs() + passes * rg.abs()).double()
                ratio = float((err / bound).max())
                worst[(passes, n)] = ratio
                assert ratio <= 1.0, f"{n} x{passes}: err/bound {ratio:.3f}"
        k, v = max(worst.items(), key=lambda kv: kv[1])
        print(f"[accumulate vs oracle {cfg_name}/{image}/{mode}/rc{recompute}] worst err/bound {v:.3f} ({k[1]} x{k[0]})")


@pytest.mark.parametrize("recompute", [0, 1])
@pytest.mark.parametrize("mode", ah.TRAIN_MODES)
def test_accumulate_vs_overwrite_same_mode(pkg, hiplib, mode, recompute):
    """|acc - (G0 + g)| <= 2^-22 * (|G0| + |g|) element-wise against the same mode's accumulate = 0 run."""
    B, (H, W) = 3, IMAGES["hostile"]["rect"]
    with Session(pkg, hiplib, "hostile", mode, recompute, seed=14) as ses:
        base = train_once(ses, B, H, W, fill=0xFF, what="accumulate = 0")
        assert_finite(base["grads"], "accumulate = 0")
        shapes = pkg.weights.param_shapes(ses.cfg)
        qb = "encoder.layers.0.self_attn.q_proj.bias"
        G0 = seeded_prior(pkg, shapes, lambda n: float(base["grads"][qb if n.endswith("k_proj.bias") else n].abs().max()), 37)
        acc = train_once(ses, B, H, W, fill=0xFF, accumulate=1, prior=G0, what="accumulate = 1")
        worst = ("", 0.0)
        for n, got in acc["grads"].items():
            g0, g = G0[n].double(), base["grads"][n].cpu().double()
            if n.endswith("k_proj.bias"):
                assert torch.equal(got.cpu(), G0[n]) and float(base["grads"][n].abs().max()) == 0.0, n
                continue
            err = (got.cpu().double() - (g0 + g)).abs()
            bound = EPS_ACC * (g0.abs() + g.abs()) + 1e-45
            ratio = float((err / bound).max())
            if ratio > worst[1]:
                worst = (n, ratio)
            assert ratio <= 1.0, f"{n}: |acc - (G0 + g)| / bound = {ratio:.3f}"
        print(f"[accumulate vs overwrite {mode}/rc{recompute}] worst err/bound {worst[1]:.3f} ({worst[0]})")


MATS = ("q_w", "k_w", "v_w", "o_w", "fc1_w", "fc2_w")
FREEZE_PATTERNS = {
    # name: (frozen sgl_layer_grads fields in EVERY block, adjacent_qkv, train_embeddings)
    "only_v_w__nonadjacent_one_slice": (("q_w", "k_w"), True, 1),
    "k_w+v_w__q_frozen": (("q_w",), True, 1),
    "separate_qkv_buffers__nonadjacent_three_slices": ((), False, 1),
    "biases+layernorm_only__no_dW_gemm": (MATS, True, 1),
    "fc1_b_frozen__fuse_cs_false": (("fc1_b",), True, 1),
    "o_b+v_b_frozen__gsum_not_requested": (("o_b", "v_b"), True, 1),
    "ln1_frozen__need_dx0_skips_dqkv_gemm": (("ln1_w", "ln1_b"), True, 0),
    "ln1_frozen__need_dx1": (("ln1_w", "ln1_b"), True, 1),
}


@pytest.mark.parametrize("mode", ah.TRAIN_MODES)
@pytest.mark.parametrize("pattern", list(FREEZE_PATTERNS))
def test_freezing_patterns_inside_a_block(pkg, oracle, hiplib, pattern, mode):
    """Per-tensor freezing: the control run hands every destination a buffer, the run under test NULL for the frozen ones;
    every surviving gradient is bit-identical (freezing a tensor must not change its neighbours) and, in fp32 / bf16x3,
    meets the oracle bar.  The separate-buffer q/k/v path runs three [D, D] TN GEMMs instead of one [3D, D]: at these token
    counts (M = 30 < 512) both take a single split, so the bar there is bitwise too."""
    frozen, adjacent, temb = FREEZE_PATTERNS[pattern]
    B, (H, W) = 2, IMAGES["hostile"]["rect"]
    with Session(pkg, hiplib, "hostile", mode, 0, seed=15) as ses:
        pres = present_for(ses, 0, temb)
        control = train_once(ses, B, H, W, fill=0xFF, present=pres, temb=temb, what="control")
        test_pres = dict(pres)
        for l in range(ses.Lyr):
            for f in frozen:
                test_pres[ah.layer_name(l, f)] = False
        got = train_once(ses, B, H, W, fill=0xFF, present=test_pres, adjacent=adjacent, temb=temb, what=pattern)
        assert set(got["grads"]) == {n for n in control["grads"] if test_pres.get(n, True)}
        assert_finite(got["grads"], pattern)
        assert_same(got["grads"], control["grads"], pattern)
        if mode in ("fp32", "bf16x3"):
            ref = Reference.get(pkg, oracle, "hostile", 15, B, H, W, 1, taps_of(ses.Lyr))
            worst = 0.0
            for n, g in got["grads"].items():
                err = float((g.cpu() - ref.grads[n]).abs().max())
                worst = max(worst, err / ref.bar(n, mode))
                assert err <= ref.bar(n, mode), f"{pattern}: {n} err {err:.3e} > {ref.bar(n, mode):.3e}"
            print(f"[freeze {pattern}/{mode}] worst err/bar {worst:.3f}")


@pytest.mark.parametrize("mode", ["fp32", "bf16x3"])
@pytest.mark.parametrize("terms", [(p, l, t) for p in (1, 0) for l in (1, 0) for t in (1, 0)],
                         ids=lambda t: "pooled%d-last%d-taplast%d" % t)
def test_upstream_gradient_combinations(pkg, oracle, hiplib, terms, mode):
    """d_pooled / d_last_hidden / d_tap_last present or NULL (the three branches at the end of sgl_backward_begin_p and
    accumulate = d_last_hidden ? 1 : 0 inside the head branch), each against the oracle with the matching loss terms
    dropped.  With all three absent every gradient is exactly zero."""
    B, (H, W) = 2, IMAGES["hostile"]["rect"]
    with Session(pkg, hiplib, "hostile", mode, 0, seed=16) as ses:
        L = ses.Lyr
        ref = Reference.get(pkg, oracle, "hostile", 16, B, H, W, 1, (L,), terms=terms)
        shadow = ses.new_shadow(0xFF)
        assert ses.prepare(shadow, full=True) == ah.OK
        run = Run(ses, B, H, W, True, 0xFF)
        assert ses.forward(run, shadow, ses.pixels(B, H, W, 1)) == ah.OK
        d_last, d_pooled, d_taps = device_upstream(ses, B, H, W, terms, taps=(L,))
        G = Grads(ses)
        st = ses.backward(run, shadow, G, d_last=d_last, d_pooled=d_pooled, d_taps=d_taps, poison_ws=0xFF)
        assert st == ah.OK
        torch.cuda.synchronize()
        ah.assert_guards(run.arenas() + G.arenas(), str(terms))
        got = G.cpu()
        assert_finite(got, str(terms))
        worst = 0.0
        for n, g in got.items():
            if not any(terms):
                assert float(g.abs().max()) == 0.0, f"{n}: no upstream gradient, yet a non-zero gradient"
                continue
            bar = ref.bar(n, mode) if float(ref.grads[n].abs().max()) > 0 or n.endswith("k_proj.bias") else 0.0
            err = float((g - ref.grads[n]).abs().max())
            worst = max(worst, err / max(bar, 1e-30))
            assert err <= bar, f"{terms}: {n} err {err:.3e} > {bar:.3e}"
        print(f"[upstream {terms}/{mode}] worst err/bar {worst:.3f}")


# =====================================================================================================================
# d. partial shadow refresh
# =====================================================================================================================
@pytest.mark.parametrize("mode", ["fp32", "bf16x3", "bf16", "fp16", "mxfp8"])
@pytest.mark.parametrize("cfg_name", ["tiny", "hostile"])
def test_partial_shadow_refresh(pkg, hiplib, cfg_name, mode):
    """Arena A: 0xFF, full prepare of W1.  Arena B: 0xFF, full prepare of W0, masters of blocks {0, L-1} and of the globals
    changed to W1's, sgl_prepare_weights_dirty with exactly those flags: byte-identical (alignment gaps keep the fill in
    both).  With any one of the flags off the arena differs from A."""
    with Session(pkg, hiplib, cfg_name, mode, seed=17) as ses:
        L = ses.Lyr
        blocks = sorted({0, L - 1})
        w0 = ses.sd
        other = pkg.weights.seeded_state_dict(ses.cfg, seed=18)

        def changed(name):
            return not name.startswith("encoder.layers.") or int(name.split(".")[2]) in blocks
        w1 = {k: (other[k] if changed(k) else v) for k, v in w0.items()}
        flags = [1 if l in blocks else 0 for l in range(L)]

        ses.set_masters(w1)
        A = ses.new_shadow(0xFF)
        assert ses.prepare(A, full=True) == ah.OK

        def refreshed(layer_flags, globals_dirty):
            ses.set_masters(w0)
            Bm = ses.new_shadow(0xFF)
            assert ses.prepare(Bm, full=True) == ah.OK
            ses.set_masters(w1)
            assert ses.prepare(Bm, dirty=layer_flags, globals_dirty=globals_dirty) == ah.OK
            torch.cuda.synchronize()
            assert Bm.guards_intact()
            return Bm
        assert torch.equal(A.payload, refreshed(flags, 1).payload), "the flagged refresh does not reproduce a full prepare"
        assert not torch.equal(A.payload, refreshed(flags, 0).payload), "globals_dirty = 0 was ignored"
        for l in blocks:
            off = list(flags)
            off[l] = 0
            assert not torch.equal(A.payload, refreshed(off, 1).payload), f"layer_dirty[{l}] = 0 was ignored"
        assert A.guards_intact()
        # the refreshed arena drives a forward without a NaN (mxfp8: the scales and the zeroed I..Ip rows included)
        run = Run(ses, 1, *IMAGES[cfg_name]["native"], False, 0xFF)
        assert ses.forward(run, refreshed(flags, 1), ses.pixels(1, *IMAGES[cfg_name]["native"], 2)) == ah.OK
        assert_finite(run.outputs(), "forward on the refreshed shadow")


# =====================================================================================================================
# e. rectangular and non-divisible images, through the raw ABI and through the package
# =====================================================================================================================
RECT_SHAPES = [("tiny", 2, 32, 48), ("tiny", 2, 64, 16), ("hostile", 2, 42, 70), ("hostile", 2, 70, 42),
               ("hostile", 2, 101, 59), ("so400m-1layer", 1, 384, 224)]


def check_vs_oracle(ref, out, grads, mode, what):
    """tests/test_encoder_gpu.py::test_forward_backward_vs_hf_golden: activations 2e-5 abs (fp32), gradients 1e-7 + 6e-5 *
    max|ref|, bf16x3 six times both."""
    x3 = 6.0 if mode == "bf16x3" else 1.0
    wa = wg = 0.0
    for k, v in out.items():
        err = float((v.cpu() - ref.out[k]).abs().max())
        wa = max(wa, err)
        assert err <= 2e-5 * x3, f"{what}: {k} err {err:.3e} > {2e-5 * x3:.1e}"
    for n, g in grads.items():
        err = float((g.cpu() - ref.grads[n]).abs().max())
        wg = max(wg, err / ref.bar(n, mode))
        assert err <= ref.bar(n, mode), f"{what}: grad {n} err {err:.3e} > {ref.bar(n, mode):.3e}"
    print(f"[{what}] worst activation err {wa:.2e} (bound {2e-5 * x3:.1e}); worst gradient err/bar {wg:.3f}")


@pytest.mark.parametrize("mode", ["fp32", "bf16x3"])
@pytest.mark.parametrize("cfg_name,B,H,W", RECT_SHAPES, ids=[f"{c}-{h}x{w}" for c, _, h, w in RECT_SHAPES])
def test_rectangular_images_raw_abi_vs_oracle(pkg, oracle, hiplib, cfg_name, B, H, W, mode):
    with Session(pkg, hiplib, cfg_name, mode, 0, seed=19) as ses:
        ref = Reference.get(pkg, oracle, cfg_name, 19, B, H, W, 1, taps_of(ses.Lyr))
        r = train_once(ses, B, H, W, fill=0xFF, what=f"{cfg_name} {H}x{W}")
        assert len(r["grads"]) == len(ref.grads)
        check_vs_oracle(ref, r["out"], r["grads"], mode, f"rect abi {cfg_name} {H}x{W} {mode}")


@pytest.mark.parametrize("recompute", [False, True])
@pytest.mark.parametrize("mode", ["fp32", "bf16x3"])
@pytest.mark.parametrize("cfg_name,B,H,W", RECT_SHAPES, ids=[f"{c}-{h}x{w}" for c, _, h, w in RECT_SHAPES])
def test_rectangular_images_package_vs_oracle(pkg, oracle, hiplib, cfg_name, B, H, W, mode, recompute):
    cfg = pkg.get_config(cfg_name)
    L = cfg.num_hidden_layers
    ref = Reference.get(pkg, oracle, cfg_name, 19, B, H, W, 1, taps_of(L))
    model = pkg.SiglipVisionModelHIP(cfg, compute_dtype=mode, recompute=recompute)
    model.load_state_dict(pkg.weights.seeded_state_dict(cfg, seed=19))
    model = model.to(DEV)
    px = pkg.weights.seeded_pixels(B, H, W, seed=1).to(DEV)
    with pytest.raises(ValueError):
        model(pixel_values=px)                         # a non-native grid without interpolate_pos_encoding
    o = model(pixel_values=px, output_hidden_states=True, interpolate_pos_encoding=True)
    M = B * ref.N
    assert o.last_hidden_state.shape == (B, ref.N, cfg.hidden_size)
    loss = (o.pooler_output * ref.up["pooled"].to(DEV)).sum() + (o.last_hidden_state * ref.up["last"].to(DEV)).sum()
    for i, u in ref.up["taps"].items():
        loss = loss + (o.hidden_states[i] * u.to(DEV)).sum()
    loss.backward()
    grads = {n: p.grad.detach() for n, p in model.named_parameters()}
    check_vs_oracle(ref, package_outputs(o, M, cfg.hidden_size), grads, mode,
                    f"rect package {cfg_name} {H}x{W} {mode} rc{int(recompute)}")


# The pooling head's token limit (csrc/kernels.h pool_attn_max_tokens; hostile has so400m's head dimension 72 and patch 14):
# 36 x 36 = 1296 tokens is the largest square grid that trains (limit 1364), 38 x 38 = 1444 the largest that infers (1488).
@pytest.mark.parametrize("mode", ["fp32", "bf16x3"])
def test_largest_trainable_square_504px_raw_abi_vs_oracle(pkg, oracle, hiplib, mode):
    B, H, W = 1, 504, 504
    with Session(pkg, hiplib, "hostile", mode, 0, seed=19) as ses:
        ref = Reference.get(pkg, oracle, "hostile", 19, B, H, W, 1, taps_of(ses.Lyr))
        r = train_once(ses, B, H, W, fill=0xFF, what=f"hostile {H}x{W}")
        assert len(r["grads"]) == len(ref.grads)
        check_vs_oracle(ref, r["out"], r["grads"], mode, f"pool limit abi hostile {H}x{W} {mode}")


@pytest.mark.parametrize("mode", ["fp32", "bf16x3"])
def test_largest_inference_square_532px_raw_abi_vs_oracle(pkg, oracle, hiplib, mode):
    B, H, W = 1, 532, 532
    with Session(pkg, hiplib, "hostile", mode, 0, seed=19) as ses:
        x = pkg.weights.seeded_pixels(B, H, W, seed=1)
        with torch.no_grad():
            want = oracle.vision_forward(x, pkg.weights.seeded_state_dict(ses.cfg, seed=19), ses.cfg, True, True)
        run = infer_once(ses, B, H, W, fill=0xFF, what=f"hostile {H}x{W} inference")
        out = run.outputs(pooled=True)
        x3 = 6.0 if mode == "bf16x3" else 1.0
        N, D = 38 * 38, ses.D
        for k, w in (("pooled", want["pooler_output"]), ("last", want["last_hidden_state"].reshape(B * N, D))):
            err = float((out[k].cpu() - w).abs().max())
            print(f"[pool limit abi hostile {H}x{W} {mode}] {k} err {err:.2e} (bound {2e-5 * x3:.1e})")
            assert err <= 2e-5 * x3, f"{k} err {err:.3e} > {2e-5 * x3:.1e}"


def test_largest_token_counts_run_in_plain_bf16(pkg, hiplib):
    """The oracle bars above exist for fp32 and bf16x3 only (Reference.bar), so the pool_attn<bf16> instantiations are run
    at the same two sizes without them: 504 px training and 532 px inference in plain bf16 write no guard, give finite
    outputs and gradients, and give the same bits when run a second time (every reduction has a fixed order)."""
    with Session(pkg, hiplib, "hostile", "bf16", 0, seed=19) as ses:
        a = train_once(ses, 1, 504, 504, fill=0xFF, what="hostile 504x504 bf16")
        b = train_once(ses, 1, 504, 504, fill=0xFF, what="hostile 504x504 bf16, again")
        assert_finite(a["out"], "504 px bf16 outputs")
        assert_finite(a["grads"], "504 px bf16 gradients")
        assert_same(a["out"], b["out"], "504 px bf16 outputs, two runs")
        assert_same(a["grads"], b["grads"], "504 px bf16 gradients, two runs")
        o1 = infer_once(ses, 1, 532, 532, fill=0xFF, what="hostile 532x532 bf16 inference").outputs(pooled=True)
        o2 = infer_once(ses, 1, 532, 532, fill=0xFF, what="hostile 532x532 bf16 inference, again").outputs(pooled=True)
        assert_finite(o1, "532 px bf16 outputs")
        assert_same(o1, o2, "532 px bf16 outputs, two runs")


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_raw_abi_refuses_546px_and_touches_nothing(pkg, hiplib, mode):
    """39 x 39 = 1521 tokens through sgl_forward, every arena filled with 0xFF first (sized for two 532 px images, which
    is more than one 546 px image needs): SGL_ERR_BAD_SHAPE, and after a synchronize every byte of the workspace, the
    hidden states and both outputs is still 0xFF.  The same call on a context without the head runs."""
    with Session(pkg, hiplib, "hostile", mode, 0, seed=19) as ses:
        shadow = ses.new_shadow(0xFF)
        assert ses.prepare(shadow, full=True) == ah.OK
        run = Run(ses, 2, 532, 532, False, 0xFF)
        run.B, run.H, run.W = 1, 546, 546
        px = ses.pixels(1, 546, 546, 1)
        torch.cuda.synchronize()
        assert ses.forward(run, shadow, px) == ah.ERR_BAD_SHAPE
        torch.cuda.synchronize()
        for name, a in run.arenas():
            assert a.untouched() and a.guards_intact(), f"`{name}` was written by a refused sgl_forward"
    with Session(pkg, hiplib, "hostile", mode, 0, use_head=0, seed=19) as ses:
        run = infer_once(ses, 1, 546, 546, fill=0xFF, pooled=False, what="hostile 546x546 without the head")
        assert_finite(run.outputs(pooled=False), "546 px without the head")


def test_raw_abi_refuses_token_limit_plus_one_and_touches_nothing(pkg, hiplib):
    """so400m-1layer, bf16 inference on one-patch-high images (14 x 14 px: one token each), B = 493 448 = the token limit
    + 1: its fc2 operand `a` [M][4352] bf16 would be the first of 2^32 bytes, which the GEMM refuses.  sgl_forward returns
    SGL_ERR_BAD_SHAPE from its prologue: every arena (sized for 64 such images, filled with 0xFF) keeps every byte and its
    guards.  The limit itself is accepted by sgl_query_sizes; through the package the refusal is SglError from
    sgl_query_sizes (host arithmetic, nothing launched)."""
    limit = 493_447
    with Session(pkg, hiplib, "so400m-1layer", "bf16", 0, seed=19) as ses:
        assert ses.sizes(limit, 14, 14, False)[0] == ah.OK
        assert ses.sizes(limit + 1, 14, 14, False)[0] == ah.ERR_BAD_SHAPE
        shadow = ses.new_shadow(0xFF)
        assert ses.prepare(shadow, full=True) == ah.OK
        run = Run(ses, 64, 14, 14, False, 0xFF)
        run.B = limit + 1
        px = ses.pixels(64, 14, 14, 1)          # never read: the shape is refused (and the arenas are too small) first
        torch.cuda.synchronize()
        assert ses.forward(run, shadow, px) == ah.ERR_BAD_SHAPE
        torch.cuda.synchronize()
        for name, a in run.arenas():
            assert a.untouched() and a.guards_intact(), f"`{name}` was written by a refused sgl_forward"
    cfg = pkg.get_config("so400m-1layer")
    model = pkg.SiglipVisionModelHIP(cfg, compute_dtype="bf16").to(DEV).eval()
    x = torch.empty(limit + 1, 3, 14, 14, device=DEV)      # 1.16 GB; refused before it is read
    with torch.no_grad(), pytest.raises(pkg.lib.SglError, match="sgl_query_sizes: bad shape"):
        model(pixel_values=x, interpolate_pos_encoding=True)
    del x, model
    torch.cuda.empty_cache()


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_package_refuses_546px_before_any_launch(pkg, hiplib, mode):
    """39 x 39 = 1521 tokens is above the pooling head's 1488: the package raises its status error, and raises it from
    sgl_query_sizes (host arithmetic, the first ABI call of a forward), so no forward entry point was entered and nothing
    was launched; 532 px right below it still runs.  Training refuses 518 px the same way."""
    cfg = pkg.get_config("hostile")
    model = pkg.SiglipVisionModelHIP(cfg, compute_dtype=mode)
    model.load_state_dict(pkg.weights.seeded_state_dict(cfg, seed=19))
    model = model.to(DEV).eval()
    px = pkg.weights.seeded_pixels(1, 546, 546, seed=1).to(DEV)
    torch.cuda.synchronize()
    with torch.no_grad():
        with pytest.raises(pkg.lib.SglError, match="sgl_query_sizes: bad shape"):
            model(pixel_values=px, interpolate_pos_encoding=True)
        torch.cuda.synchronize()
        o = model(pixel_values=px[:, :, :532, :532].contiguous(), interpolate_pos_encoding=True)
    assert o.pooler_output.shape == (1, cfg.hidden_size) and bool(torch.isfinite(o.pooler_output).all())
    with pytest.raises(pkg.lib.SglError, match="sgl_query_sizes: bad shape"):   # training: 518 px is already too many
        model.train()(pixel_values=px[:, :, :518, :518].contiguous(), interpolate_pos_encoding=True)


# =====================================================================================================================
# f. bf16x3 at >= 2048 tokens: the fp32-output gemm_nt6_kernel<Tile, 0 | 4, float, bfloat16> instantiations (0 on both tiles)
# =====================================================================================================================
def test_bf16x3_2187_tokens_vs_oracle(pkg, oracle, hiplib):
    B, H, W = 3, 384, 384
    with Session(pkg, hiplib, "so400m-1layer", "bf16x3", 0, seed=20) as ses:
        ref = Reference.get(pkg, oracle, "so400m-1layer", 20, B, H, W, 1, taps_of(ses.Lyr), interp=False)
        r = train_once(ses, B, H, W, fill=0xFF, what="so400m-1layer B=3 384px bf16x3")
        check_vs_oracle(ref, r["out"], r["grads"], "bf16x3", "bf16x3 2187 tokens")
