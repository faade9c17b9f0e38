"""GPU: the attention-gradient kernels (``sgl_op_attn_grad_probs``, ``sgl_op_pool_attn_grad_probs``), the backward hooks
(``sgl_backward_layer_pa`` / ``sgl_backward_begin_pa``) and the Python surface (``capture_attention_gradients``,
``attention_relevance``).

Raw ops: guarded, poisoned ``abi_harness.Arena`` operands; every element of every kind and mode against the float64
reference and the element-wise bounds of ``tests/attn_grad_ref.py``.  Encoder: ``attentions[l].grad`` of the real
``transformers.SiglipVisionModel`` (tests/golden/attngrad, tests/gen_golden_attn_grad.py): the strict modes to 1e-3
relative L2, the 16-bit modes to twice HF's own error under CPU autocast, per layer; the same bars for the relevance.
Everything else a capture touches must not move: outputs and gradients are compared to the bit with a run without it.
"""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest
import torch

import abi_harness as ah
import attn_grad_ref as gr
import attn_probs_ref as ar
from test_attn_grad_host import CASES, load_case, relevance_bound

pytestmark = pytest.mark.gpu

DTYPES = [ar.F32, ar.BF16, ar.BF16X3, ar.F16]
POOL_DTYPES = [ar.F32, ar.BF16, ar.F16]
SHAPES = [(2, 4, 9, 16), (1, 2, 28, 72), (2, 4, 143, 16), (1, 3, 129, 64)]
REAL = (1, 16, 729, 72)
ENC_MODES = ["fp32", "bf16x3", "bf16", "fp16"]


def pad16(dh):
    return (dh + 15) // 16 * 16


def filled(t, fill=0xFF):
    """A guarded arena whose payload is exactly t's bytes."""
    t = t.contiguous()
    a = ah.Arena(t.numel() * t.element_size(), fill)
    a.payload.copy_(t.view(torch.uint8).reshape(-1).cuda())
    return a


@functools.lru_cache(maxsize=None)
def op_case(shape, dtype):
    """Inputs of one (shape, dtype), made once and shared (never modified)."""
    B, H, N, dh = shape
    return gr.inputs(B, H, N, dh, dtype, seed=23 + N + dh)


class OpRun:
    def __init__(self, lib, shape, dtype, q, k, v, dout, lse):
        self.lib, self.shape, self.dtype = lib, shape, dtype
        self.DP = pad16(shape[3])
        self.ins = [filled(ar.pad_heads(q, self.DP)), filled(ar.pad_heads(k, self.DP)), filled(ar.pad_heads(v, self.DP)),
                    filled(gr.token_major(dout)), filled(lse)]
        self.before = [a.payload.clone() for a in self.ins]

    def run(self, kind, mode):
        B, H, N, dh = self.shape
        shape = (B, N, N) if mode else (B, H, N, N)
        out = ah.Arena(int(np.prod(shape)) * 4, 0xFF)
        q, k, v, g, lse = self.ins
        st = self.lib.sgl_op_attn_grad_probs(self.dtype, q.ptr, k.ptr, v.ptr, g.ptr, lse.ptr, out.ptr, B, H, N, dh,
                                             self.DP, kind, mode, ah.stream())
        assert st == ah.OK, f"status {st}"
        torch.cuda.synchronize()
        ah.assert_guards(list(zip(("q", "k", "v", "dout", "lse"), self.ins)) + [("out", out)], "sgl_op_attn_grad_probs")
        for a, b in zip(self.ins, self.before):
            assert torch.equal(a.payload, b), "an input was written"
        return out.f32(*shape).cpu()


def check_op(lib, shape, dtype):
    q, k, v, dout, lse = op_case(shape, dtype)
    r = OpRun(lib, shape, dtype, q, k, v, dout, lse)
    name = f"{ar.DT_NAME[dtype]} {shape}"
    for kind in gr.KINDS:
        ref, bound = gr.grad_probs_ref(q, k, v, dout, lse, dtype, kind)
        full = r.run(kind, ar.FULL)
        worst = gr.worst_ratio(full, ref, bound)
        mean = r.run(kind, ar.HEAD_MEAN)
        m_ref, m_bound = gr.head_mean_ref(ref, bound)
        wm = gr.worst_ratio(mean, m_ref, m_bound)
        o_ref, o_bound = gr.head_mean_of_full(full)
        wo = gr.worst_ratio(mean, o_ref, o_bound)
        print(f"{name} {gr.KIND_NAME[kind]}: worst |err| / bound FULL {worst:.3f}, HEAD_MEAN {wm:.3f}, "
              f"HEAD_MEAN against the mean of FULL / (H 2^-24) {wo:.3f}")
        assert worst <= 1.0 and wm <= 1.0 and wo <= 1.0
        assert torch.equal(full, r.run(kind, ar.FULL)) and torch.equal(mean, r.run(kind, ar.HEAD_MEAN))
        if kind == gr.RELEVANCE:
            assert float(full.min()) >= 0.0 and float(mean.min()) >= 0.0


@pytest.mark.parametrize("dtype", DTYPES, ids=[ar.DT_NAME[d] for d in DTYPES])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_op_against_float64(hiplib, shape, dtype):
    check_op(hiplib, shape, dtype)


def test_op_real_size_bf16(hiplib):
    check_op(hiplib, REAL, ar.BF16)


@pytest.mark.parametrize("dtype", POOL_DTYPES, ids=[ar.DT_NAME[d] for d in POOL_DTYPES])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_pool_op_against_float64(hiplib, shape, dtype):
    B, H, N, dh = shape
    DP = pad16(dh)
    g = torch.Generator().manual_seed(N + dh)
    v = torch.randn(B, H, N, dh, generator=g).to(ar.TORCH_DT[dtype])
    probs = torch.softmax(torch.randn(B, H, N, generator=g), -1)
    dout = torch.randn(B, H, dh, generator=g)
    ins = [filled(ar.pad_heads(v, DP)), filled(probs), filled(dout.reshape(B, H * dh))]
    before = [a.payload.clone() for a in ins]

    def run(kind, mode):
        shape_o = (B, N) if mode else (B, H, N)
        out = ah.Arena(int(np.prod(shape_o)) * 4, 0xFF)
        st = hiplib.sgl_op_pool_attn_grad_probs(dtype, ins[0].ptr, ins[1].ptr, ins[2].ptr, out.ptr, B, H, N, dh, DP, kind,
                                                mode, ah.stream())
        assert st == ah.OK, st
        torch.cuda.synchronize()
        ah.assert_guards(list(zip(("V", "probs", "dout"), ins)) + [("out", out)], "sgl_op_pool_attn_grad_probs")
        for a, b in zip(ins, before):
            assert torch.equal(a.payload, b), "an input was written"
        return out.f32(*shape_o).cpu()

    for kind in gr.KINDS:
        ref, bound = gr.pool_ref(v, probs, dout, kind)
        full, mean = run(kind, ar.FULL), run(kind, ar.HEAD_MEAN)
        m_ref, m_bound = gr.head_mean_ref(ref, bound)
        o_ref, o_bound = gr.head_mean_of_full(full)
        w, wm, wo = gr.worst_ratio(full, ref, bound), gr.worst_ratio(mean, m_ref, m_bound), gr.worst_ratio(mean, o_ref, o_bound)
        print(f"pool {ar.DT_NAME[dtype]} {shape} {gr.KIND_NAME[kind]}: FULL {w:.3f} HEAD_MEAN {wm:.3f} / of FULL {wo:.3f}")
        assert w <= 1.0 and wm <= 1.0 and wo <= 1.0
        assert torch.equal(full, run(kind, ar.FULL)) and torch.equal(mean, run(kind, ar.HEAD_MEAN))


@pytest.mark.parametrize("dtype", DTYPES, ids=[ar.DT_NAME[d] for d in DTYPES])
def test_head_isolation(hiplib, dtype):
    """head_dim 72, head_dim_pad 80: the last k-step's upper chunk of head h's dO row is head h + 1's first eight columns.
    NaN there must not reach head h (it is read as zero, not multiplied by V's zero pad), and must fill head h + 1's rows
    in all three kinds (a relu through fmaxf would turn them into zeros)."""
    shape = (1, 2, 28, 72)
    B, H, N, dh = shape
    q, k, v, dout, lse = op_case(shape, dtype)
    bad = dout.clone()
    bad[:, 1, :, :8] = float("nan")
    clean = OpRun(hiplib, shape, dtype, q, k, v, dout, lse)
    hot = OpRun(hiplib, shape, dtype, q, k, v, bad, lse)
    for kind in gr.KINDS:
        a, b = clean.run(kind, ar.FULL), hot.run(kind, ar.FULL)
        assert bool(torch.isfinite(b[:, 0]).all()) and torch.equal(a[:, 0], b[:, 0]), gr.KIND_NAME[kind]
        assert bool(torch.isnan(b[:, 1]).all()), gr.KIND_NAME[kind]
        assert bool(torch.isnan(hot.run(kind, ar.HEAD_MEAN)).all())


def test_op_refusals_leave_out_poisoned(hiplib):
    shape, dtype = (2, 4, 9, 16), ar.BF16
    B, H, N, dh = shape
    q, k, v, dout, lse = op_case(shape, dtype)
    r = OpRun(hiplib, shape, dtype, q, k, v, dout, lse)
    out = ah.Arena(B * H * N * N * 4, 0xFF)
    ptrs = [a.ptr for a in r.ins]

    def call(dt=dtype, p=ptrs, o=out.ptr, dims=(B, H, N, dh, r.DP), kind=gr.DP, mode=ar.FULL):
        return hiplib.sgl_op_attn_grad_probs(dt, p[0], p[1], p[2], p[3], p[4], o, *dims, kind, mode, ah.stream())

    assert call(o=None) == ah.ERR_NULL
    for i in range(5):
        assert call(p=ptrs[:i] + [None] + ptrs[i + 1:]) == ah.ERR_NULL
    assert call(dims=(B, H, 0, dh, r.DP)) == ah.ERR_BAD_SHAPE and call(dims=(B, H, N, dh, 32)) == ah.ERR_BAD_SHAPE
    assert call(dt=4) == ah.ERR_UNSUPPORTED and call(kind=3) == ah.ERR_UNSUPPORTED and call(mode=2) == ah.ERR_UNSUPPORTED
    assert call(p=[ptrs[0], ptrs[1], ptrs[2] + 2, ptrs[3], ptrs[4]]) == ah.ERR_UNSUPPORTED
    assert call(p=[ptrs[0], ptrs[1], ptrs[2], ptrs[3] + 2, ptrs[4]]) == ah.ERR_UNSUPPORTED
    pv, pp, pd = filled(ar.pad_heads(v, r.DP)), filled(torch.rand(B, H, N)), filled(torch.randn(B, H * dh))

    def pool(V=pv.ptr, probs=pp.ptr, d=pd.ptr, o=out.ptr, dt=dtype, dims=(B, H, N, dh, r.DP), kind=gr.DP, mode=ar.FULL):
        return hiplib.sgl_op_pool_attn_grad_probs(dt, V, probs, d, o, *dims, kind, mode, ah.stream())

    assert pool(V=None) == ah.ERR_NULL and pool(probs=None) == ah.ERR_NULL and pool(d=None) == ah.ERR_NULL
    assert pool(o=None) == ah.ERR_NULL
    assert pool(dims=(B, H, N, 12, 16)) == ah.ERR_BAD_SHAPE and pool(dims=(0, H, N, dh, r.DP)) == ah.ERR_BAD_SHAPE
    assert pool(dt=ar.BF16X3) == ah.ERR_UNSUPPORTED and pool(V=pv.ptr + 2) == ah.ERR_UNSUPPORTED
    assert pool(kind=3) == ah.ERR_UNSUPPORTED and pool(mode=-1) == ah.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert out.untouched() and out.guards_intact()
    assert call() == ah.OK and pool() == ah.OK          # and the accepted forms of the same calls run
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------
# the backward hooks on the C ABI
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_pa_entry_points_refuse_before_work_and_change_nothing(pkg, hiplib, mode):
    """A refused request leaves `out` and the workspace as they were; an accepted one writes every element of `out`, and
    the gradients and the workspace of the step are those of the plain entry points, to the bit."""
    B, H, W = 2, 59, 101
    with ah.Session(pkg, hiplib, "hostile", mode) as ses:
        shadow = ses.new_shadow()
        assert ses.prepare(shadow, full=True) == ah.OK
        L, Hh = ses.Lyr, ses.cfg.num_attention_heads
        N = ses.geometry(B, H, W)[2]
        d_pooled = (0.01 * torch.cos(torch.arange(B * ses.D, dtype=torch.float32))).view(B, ses.D).cuda()
        px = ses.pixels(B, H, W)

        def backward(reqs):
            """reqs: step -> SglAttnGradReq (L = begin).  Returns (status list, grads, workspace bytes)."""
            run = ah.Run(ses, B, H, W, train=True, fill=0xFF, kind="slots")
            assert ses.forward(run, shadow, px, kind="slots") == ah.OK
            grads = ah.Grads(ses)
            tail = (run.saved.ptr, run.saved.nbytes, run.ws.ptr, run.ws.nbytes, ah.stream())
            wsg = (ses.ctx, C.byref(ses.w), shadow.ptr, C.byref(grads.struct))
            ref = lambda s: C.byref(reqs[s]) if s in reqs else None
            sts = [hiplib.sgl_backward_begin_pa(*wsg, B, H, W, run.hidden_ptr(L), None, d_pooled.data_ptr(), None, *tail,
                                                ref(L))]
            for l in range(L - 1, -1, -1):
                sts.append(hiplib.sgl_backward_layer_pa(*wsg, l, B, H, W, run.hidden_ptr(l), None, 1, *tail, ref(l)))
            torch.cuda.synchronize()
            ah.assert_guards(run.arenas() + grads.arenas(), "sgl_backward_*_pa")
            return sts, grads.gpu(), run.ws.payload.clone(), run

        plain_sts, g_plain, ws_plain, run = backward({})
        assert all(s == ah.OK for s in plain_sts)
        # refusals on a live run: nothing moves
        out = ah.Arena(B * Hh * N * N * 4, 0xFF)
        run.ws.poison(0x5A)
        tail = (run.saved.ptr, run.saved.nbytes, run.ws.ptr, run.ws.nbytes, ah.stream())
        grads = ah.Grads(ses)
        wsg = (ses.ctx, C.byref(ses.w), shadow.ptr, C.byref(grads.struct))
        R = pkg.lib.SglAttnGradReq
        for req, want in ((R(None, out.nbytes, 0, 0), ah.ERR_NULL), (R(out.ptr, out.nbytes, 3, 0), ah.ERR_UNSUPPORTED),
                          (R(out.ptr, out.nbytes, 0, 2), ah.ERR_UNSUPPORTED),
                          (R(out.ptr, B * Hh * N * N * 4 - 1, 0, 0), ah.ERR_WORKSPACE),
                          (R(out.ptr, B * N * N * 4 - 1, 2, 1), ah.ERR_WORKSPACE)):
            assert hiplib.sgl_backward_layer_pa(*wsg, L - 1, B, H, W, run.hidden_ptr(L - 1), None, 1, *tail,
                                                C.byref(req)) == want
        for req, want in ((R(None, out.nbytes, 0, 0), ah.ERR_NULL), (R(out.ptr, out.nbytes, -1, 0), ah.ERR_UNSUPPORTED),
                          (R(out.ptr, B * Hh * N * 4 - 1, 0, 0), ah.ERR_WORKSPACE)):
            assert hiplib.sgl_backward_begin_pa(*wsg, B, H, W, run.hidden_ptr(L), None, d_pooled.data_ptr(), None, *tail,
                                                C.byref(req)) == want
        assert hiplib.sgl_backward_begin_pa(*wsg, B, H, W, run.hidden_ptr(L), None, None, None, *tail,
                                            C.byref(R(out.ptr, out.nbytes, 0, 0))) == ah.ERR_UNSUPPORTED
        torch.cuda.synchronize()
        assert out.untouched() and out.guards_intact() and bool((run.ws.payload == 0x5A).all())
        assert all(a.untouched() for _, a in grads.arenas())
        # accepted requests on every step: exact-size outputs, all written, nothing else differs
        outs = {s: ah.Arena(B * (N if s == L else N * N) * 4, 0xFF) for s in range(L + 1)}
        sts, g_req, ws_req, _ = backward({s: R(a.ptr, a.nbytes, gr.RELEVANCE, ar.HEAD_MEAN) for s, a in outs.items()})
        assert all(s == ah.OK for s in sts)
        for s, a in outs.items():
            t = a.f32(-1)
            assert a.guards_intact() and bool(torch.isfinite(t).all()) and float(t.min()) >= 0.0, s
        assert torch.equal(ws_plain, ws_req)
        assert g_plain.keys() == g_req.keys()
        for n in g_plain:          # bit patterns: the embedding destinations keep their NaN fill (no sgl_backward_embed here)
            assert torch.equal(g_plain[n].view(torch.int32), g_req[n].view(torch.int32)), n
    for kw in (dict(recompute=1), dict(use_head=0)):
        with ah.Session(pkg, hiplib, "hostile", mode, **kw) as ses:
            shadow = ses.new_shadow()
            assert ses.prepare(shadow, full=True) == ah.OK
            run = ah.Run(ses, B, H, W, train=True, fill=0xFF, kind="slots")
            assert ses.forward(run, shadow, ses.pixels(B, H, W), kind="slots", pooled=not kw.get("use_head", 1) == 0) == ah.OK
            grads = ah.Grads(ses)
            out = ah.Arena(B * N * N * 4, 0xFF)
            req = pkg.lib.SglAttnGradReq(out.ptr, out.nbytes, 0, 1)
            tail = (run.saved.ptr, run.saved.nbytes, run.ws.ptr, run.ws.nbytes, ah.stream())
            wsg = (ses.ctx, C.byref(ses.w), shadow.ptr, C.byref(grads.struct))
            dp = torch.zeros(B, ses.D, device="cuda")
            assert hiplib.sgl_backward_begin_pa(*wsg, B, H, W, run.hidden_ptr(ses.Lyr), None, dp.data_ptr(), None, *tail,
                                                C.byref(req)) == ah.ERR_UNSUPPORTED
            if kw.get("recompute"):
                assert hiplib.sgl_backward_layer_pa(*wsg, ses.Lyr - 1, B, H, W, run.hidden_ptr(ses.Lyr - 1), None, 1, *tail,
                                                    C.byref(req)) == ah.ERR_UNSUPPORTED
            torch.cuda.synchronize()
            assert out.untouched()


# ---------------------------------------------------------------------------------------------------------------
# encoder against HF
# ---------------------------------------------------------------------------------------------------------------
def case_setup(pkg, name):
    meta, grads = load_case(name)
    cfg = pkg.get_config(str(meta["meta.config"]))
    seed = int(meta["meta.seed"])
    sd = pkg.weights.seeded_state_dict(cfg, seed=seed)
    x = pkg.weights.seeded_pixels(int(meta["meta.batch"]), int(meta["meta.res_h"]), int(meta["meta.res_w"]), seed=seed + 1000)
    return meta, grads, cfg, sd, x


def make_model(pkg, cfg, sd, mode):
    m = pkg.SiglipVisionModelHIP(cfg, compute_dtype=mode).to("cuda")
    m.load_state_dict(sd)
    return m


def l2rel(a, ref):
    return float((a.double() - ref.double()).norm() / ref.double().norm())


@pytest.mark.parametrize("mode", ENC_MODES)
@pytest.mark.parametrize("name", CASES)
def test_encoder_gradients_against_hf(pkg, hiplib, name, mode):
    """kind "grad", all heads: attentions[l].grad of HF, per layer; the pooling head's gradient; and
    model.attention_relevance against the float64 relevance composed from HF's maps and gradients."""
    meta, grads, cfg, sd, x = case_setup(pkg, name)
    m = make_model(pkg, cfg, sd, mode)
    w = torch.from_numpy(meta["score.w"]).cuda()
    xg = x.cuda()
    with m.capture_attention_gradients(heads="all", kind="grad") as cap:
        out = m(pixel_values=xg, interpolate_pos_encoding=True)
        (out.pooler_output @ w).sum().backward()
    torch.cuda.synchronize()
    strict = mode in ("fp32", "bf16x3")
    tag = "bf16ac." if mode == "bf16" else "fp16ac."
    assert sorted(cap.maps) == list(range(len(grads)))
    for l, ref in enumerate(grads):
        a = cap.maps[l].cpu()
        assert a.shape == ref.shape and a.dtype == torch.float32 and not a.requires_grad
        rel = l2rel(a, ref)
        if strict:
            print(f"{name} {mode} layer {l}: l2rel {rel:.3e}")
            assert rel <= 1e-3
        else:
            yard = float(meta[tag + "attn_grad.l2rel"][l])
            print(f"{name} {mode} layer {l}: l2rel {rel:.3e} = {rel / yard:.2f} x HF autocast ({yard:.3e})")
            assert rel <= 2 * yard
    pool_ref = torch.from_numpy(meta["pooling_grad"])
    prel = l2rel(cap.pooling.cpu(), pool_ref)
    print(f"{name} {mode} pooling gradient: l2rel {prel:.3e}")
    assert cap.pooling.shape == pool_ref.shape
    if strict:
        assert prel <= 1e-3
    r = m.attention_relevance(xg, lambda o: o.pooler_output @ w)
    torch.cuda.synchronize()
    ref = torch.from_numpy(meta["relevance"])
    P = cfg.patch_size
    assert r.shape == (xg.shape[0], xg.shape[2] // P, xg.shape[3] // P) and not r.requires_grad and r.dtype == torch.float32
    rrel = l2rel(r.reshape(ref.shape).cpu(), ref)
    if strict:
        print(f"{name} {mode} relevance: l2rel {rrel:.3e}")
        assert rrel <= 1e-3
    else:
        yard = float(meta[tag + "relevance.l2rel"])
        print(f"{name} {mode} relevance: l2rel {rrel:.3e} = {rrel / yard:.2f} x HF autocast ({yard:.3e})")
        assert rrel <= 2 * yard


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
@pytest.mark.parametrize("name", ["tiny_208x176", "hostile_59x101"])
def test_capture_changes_nothing_else(pkg, hiplib, name, mode):
    """Outputs, parameter gradients and the pixel gradient of a backward under a capture equal the same backward without
    it, to the bit; attention_relevance leaves every p.grad None and the caller's tensor alone."""
    meta, grads, cfg, sd, x = case_setup(pkg, name)
    taps = (1, cfg.num_hidden_layers)

    def run(capture):
        m = make_model(pkg, cfg, sd, mode)
        xg = x.cuda().requires_grad_(True)
        cm = m.capture_attention_gradients() if capture else None
        if cm is not None:
            cm.__enter__()
        out = m(pixel_values=xg, hidden_state_ids=taps, interpolate_pos_encoding=True)
        loss = out.pooler_output.square().sum() + out.last_hidden_state.square().mean() + \
            sum(h.square().mean() for h in out.hidden_states)
        loss.backward()
        if cm is not None:
            cm.__exit__(None, None, None)
        torch.cuda.synchronize()
        return out, {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}, xg.grad.clone(), cm

    plain, g_plain, px_plain, _ = run(False)
    capt, g_capt, px_capt, cap = run(True)
    assert torch.equal(capt.pooler_output, plain.pooler_output)
    assert torch.equal(capt.last_hidden_state, plain.last_hidden_state)
    for a, b in zip(capt.hidden_states, plain.hidden_states):
        assert torch.equal(a, b)
    assert g_plain.keys() == g_capt.keys() and len(g_plain) > 0
    for n in g_plain:
        assert torch.equal(g_plain[n], g_capt[n]), n
    assert torch.equal(px_plain, px_capt)
    assert sorted(cap.maps) == list(range(cfg.num_hidden_layers)) and cap.pooling is not None
    m = make_model(pkg, cfg, sd, mode)
    xg = x.cuda()
    before = xg.clone()
    r = m.attention_relevance(xg, lambda o: o.pooler_output[:, 1])
    torch.cuda.synchronize()
    assert all(p.grad is None for p in m.parameters())
    assert torch.equal(xg, before) and xg.grad is None and not xg.requires_grad
    assert bool(torch.isfinite(r).all()) and float(r.min()) >= 0.0


# ---------------------------------------------------------------------------------------------------------------
# surface
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["bf16", "bf16x3"])
def test_layer_subsets_sink_and_relevance(pkg, hiplib, mode):
    name = "tiny_208x176"
    meta, grads, cfg, sd, x = case_setup(pkg, name)
    m = make_model(pkg, cfg, sd, mode)
    L, Hh = cfg.num_hidden_layers, cfg.num_attention_heads
    score = lambda o: o.pooler_output[:, 3]

    def capture(xg, **kw):
        with m.capture_attention_gradients(**kw) as cap:
            score(m(pixel_values=xg, interpolate_pos_encoding=True)).sum().backward()
        torch.cuda.synchronize()
        m.zero_grad(set_to_none=True)
        return cap

    xg = x.cuda()
    full = capture(xg, heads="all")
    mean = capture(xg)
    assert sorted(full.maps) == sorted(mean.maps) == list(range(L))
    N = full.maps[0].shape[-1]
    for l in range(L):
        assert full.maps[l].shape == (xg.shape[0], Hh, N, N) and mean.maps[l].shape == (xg.shape[0], N, N)
        ref, bound = gr.head_mean_of_full(full.maps[l].cpu())
        assert gr.worst_ratio(mean.maps[l].cpu(), ref, bound) <= 1.0
        assert float(mean.maps[l].min()) >= 0.0
    assert full.pooling.shape == (xg.shape[0], Hh, N) and mean.pooling.shape == (xg.shape[0], N)
    # subsets and negative indices: the same bits, only the blocks asked for
    sub = capture(xg, layers=[-1, 0])
    assert sorted(sub.maps) == [0, L - 1]
    assert torch.equal(sub.maps[0], mean.maps[0]) and torch.equal(sub.maps[L - 1], mean.maps[L - 1])
    for kind in ("grad", "prob_grad"):
        other = capture(xg, layers=[1], heads="all", kind=kind)
        assert list(other.maps) == [1] and not torch.equal(other.maps[1], full.maps[1])
    pg = capture(xg, layers=[1], heads="all", kind="prob_grad").maps[1]
    assert torch.equal(torch.relu(pg), full.maps[1])          # relevance is the relu of prob_grad, bit for bit
    # sink: blocks in descending order, one buffer, the bits of the stored maps
    seen, ptrs = [], set()

    def sink(layer, t):
        seen.append((layer, t.clone()))
        ptrs.add(t.data_ptr())

    sunk = capture(xg, sink=sink)
    assert [l for l, _ in seen] == list(range(L - 1, -1, -1)) and len(ptrs) == 1 and sunk.maps == {}
    for l, t in seen:
        assert torch.equal(t, mean.maps[l])
    assert torch.equal(sunk.pooling, mean.pooling)
    # attention_relevance = heads.attention_relevance of the separately captured maps, up to the fp32 rounding of the two
    # summation orders (row vector down the blocks against the matrix product): relevance_bound for each, all terms >= 0
    r = m.attention_relevance(xg, score)
    want = pkg.heads.attention_relevance([mean.maps[l] for l in range(L)], pooling=mean.pooling)
    tol = 2 * relevance_bound([mean.maps[l] for l in range(L)])
    dev = ((r.reshape(want.shape).double() - want.double()).abs() / want.double().clamp_min(1e-300)).max()
    print(f"{mode}: attention_relevance against heads.attention_relevance: worst relative {float(dev):.3e} (bound {tol:.3e})")
    assert float(dev) <= tol
    with pytest.raises(ValueError):
        m.capture_attention_gradients(kind="saliency")
    with pytest.raises(ValueError):
        m.capture_attention_gradients(heads="max")
    with pytest.raises(RuntimeError):
        m.capture_attention_gradients(layers=[L])


def test_frozen_prefix_and_refusals(pkg, hiplib):
    name = "tiny_48"
    meta, grads, cfg, sd, x = case_setup(pkg, name)
    m = make_model(pkg, cfg, sd, "bf16")
    L = cfg.num_hidden_layers
    m.embeddings.requires_grad_(False)
    m.encoder.layers[0].requires_grad_(False)
    xg = x.cuda()
    with pytest.raises(RuntimeError, match=r"pixel_values\.requires_grad_\(\)"):
        with m.capture_attention_gradients():
            m(pixel_values=xg, interpolate_pos_encoding=True).pooler_output.sum().backward()
    m.zero_grad(set_to_none=True)
    with m.capture_attention_gradients(layers=[-1]) as cap:          # a block that trains is reached
        m(pixel_values=xg, interpolate_pos_encoding=True).pooler_output.sum().backward()
    assert list(cap.maps) == [L - 1]
    with m.capture_attention_gradients() as cap:                     # and with an input gradient every block is
        m(pixel_values=xg.clone().requires_grad_(True), interpolate_pos_encoding=True).pooler_output.sum().backward()
    assert sorted(cap.maps) == list(range(L))
    with pytest.raises(RuntimeError, match="already active"):
        with m.capture_attention_gradients(layers=[]):
            with m.capture_attention_gradients(layers=[]):
                pass
    with m.capture_attention_gradients(layers=[]):                   # the failed nesting left nothing behind
        pass
    rc = pkg.SiglipVisionModelHIP(cfg, compute_dtype="bf16", recompute=True).to("cuda")
    with pytest.raises(RuntimeError, match="recompute=True"):
        rc.capture_attention_gradients()
    with pytest.raises(RuntimeError, match="recompute=True"):
        rc.attention_relevance(xg, lambda o: o.pooler_output[:, 0])
    mx = pkg.SiglipVisionModelHIP(cfg, compute_dtype="mxfp8").to("cuda")
    with pytest.raises(RuntimeError, match="mxfp8"):
        mx.capture_attention_gradients()
    # a model without the pooling head: the block maps exist, the pooling row does not
    nh = pkg.SiglipVisionModelHIP(dataclasses.replace(cfg, vision_use_head=False), compute_dtype="bf16").to("cuda")
    nh.load_state_dict({k: v for k, v in sd.items() if ".head." not in "." + k})
    with pytest.raises(RuntimeError, match=r"heads\.attention_relevance"):
        nh.attention_relevance(xg, lambda o: o.last_hidden_state.mean((1, 2)))
    with nh.capture_attention_gradients() as cap:
        nh(pixel_values=xg, interpolate_pos_encoding=True).last_hidden_state.square().sum().backward()
    assert sorted(cap.maps) == list(range(L)) and cap.pooling is None
    R = pkg.heads.attention_relevance([cap.maps[l] for l in range(L)])
    assert R.shape == cap.maps[0].shape and bool(torch.isfinite(R).all())
    # the score did not go through pooler_output on a model WITH the head: said so
    with pytest.raises(RuntimeError, match="pooler_output"):
        m.attention_relevance(xg, lambda o: o.last_hidden_state.mean((1, 2)))


def test_relevance_under_torch_compile_is_a_graph_break(pkg, hiplib):
    name = "tiny_48"
    meta, grads, cfg, sd, x = case_setup(pkg, name)
    m = make_model(pkg, cfg, sd, "bf16")
    xg = x.cuda()
    score = lambda o: o.pooler_output[:, 1]
    eager = m.attention_relevance(xg, score)

    def f(t):
        return m.attention_relevance(t, score) * 1.0

    got = torch.compile(f)(xg)
    assert torch.equal(got, eager)
    with torch.no_grad():
        assert torch.equal(torch.compile(m)(pixel_values=xg, interpolate_pos_encoding=True).pooler_output,
                           m(pixel_values=xg, interpolate_pos_encoding=True).pooler_output)
