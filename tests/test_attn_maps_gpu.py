"""GPU: the attention-probability kernel (``sgl_op_attn_probs``), the encoder entry point (``sgl_attention_probs``) and the
Python surface (``output_attentions=True``, ``attention_rollout``).

Raw op: guarded, poisoned ``abi_harness.Arena`` operands; every element against the float64 reference and the element-wise
bounds of ``tests/attn_probs_ref.py``.  Encoder: the maps of the real ``transformers.SiglipVisionModel``
(tests/golden/attn, tests/gen_golden_attn.py): the strict modes to 1e-3 absolute, the 16-bit modes to twice HF's own error
under CPU autocast, per layer.  Everything else the flag touches must not move: outputs and gradients are compared to the
bit with a call without it.
"""
import functools

import numpy as np
import pytest
import torch

import abi_harness as ah
import attn_probs_ref as ar
from test_attn_maps_host import CASES, load_case

pytestmark = pytest.mark.gpu

DTYPES = [ar.F32, ar.BF16, ar.BF16X3, ar.F16]
SHAPES = [(2, 4, 9, 16), (1, 2, 28, 72), (2, 4, 143, 16), (1, 3, 129, 64)]
REAL = (1, 16, 729, 72)
ENC_MODES = ["fp32", "bf16x3", "bf16", "fp16"]


def pad16(dh):
    return (dh + 15) // 16 * 16


@functools.lru_cache(maxsize=None)
def op_case(shape, dtype):
    """Inputs and float64 reference of one (shape, dtype), computed once and shared (never modified)."""
    B, H, N, dh = shape
    q, k, lse = ar.inputs(B, H, N, dh, dtype, seed=17 + N + dh)
    p, bound = ar.probs_ref(q, k, lse, dtype)
    return q, k, lse, p, bound


def filled(t, fill=0xFF):
    """A guarded arena whose payload is exactly t's bytes."""
    t = t.contiguous()
    a = ah.Arena(t.numel() * t.element_size(), fill)
    a.payload.copy_(t.view(torch.uint8).reshape(-1).cuda())
    return a


class OpRun:
    def __init__(self, lib, shape, dtype, q, k, lse):
        self.lib, self.shape, self.dtype = lib, shape, dtype
        B, H, N, dh = shape
        self.DP = pad16(dh)
        self.q, self.k, self.lse = filled(ar.pad_heads(q, self.DP)), filled(ar.pad_heads(k, self.DP)), filled(lse)
        self.before = [a.payload.clone() for a in (self.q, self.k, self.lse)]

    def run(self, mode, lse=None):
        B, H, N, dh = self.shape
        out = ah.Arena((B * N * N if mode else B * H * N * N) * 4, 0xFF)
        st = self.lib.sgl_op_attn_probs(self.dtype, self.q.ptr, self.k.ptr, (self.lse if lse is None else lse).ptr,
                                        out.ptr, B, H, N, dh, self.DP, mode, ah.stream())
        assert st == ah.OK, f"status {st}"
        torch.cuda.synchronize()
        ah.assert_guards([("q", self.q), ("k", self.k), ("lse", self.lse), ("out", out)], "sgl_op_attn_probs")
        for a, b in zip((self.q, self.k, self.lse), self.before):
            assert torch.equal(a.payload, b), "an input was written"
        return out.f32(*((B, N, N) if mode else (B, H, N, N))).cpu(), out


def check_op(lib, shape, dtype):
    q, k, lse, p, bound = op_case(shape, dtype)
    H = shape[1]
    r = OpRun(lib, shape, dtype, q, k, lse)
    full, _ = r.run(ar.FULL)
    worst = ar.worst_ratio(full, p, bound)
    print(f"{ar.DT_NAME[dtype]} {shape} FULL worst |err| / bound = {worst:.3f}")
    assert worst <= 1.0
    # HEAD_MEAN: H - 1 additions and one division of the same fp32 values; twice, to the bit
    mean, _ = r.run(ar.HEAD_MEAN)
    mean2, _ = r.run(ar.HEAD_MEAN)
    assert torch.equal(mean, mean2)
    m_ref, m_bound = ar.head_mean_ref(full)
    wm = ar.worst_ratio(mean, m_ref, m_bound)
    print(f"{ar.DT_NAME[dtype]} {shape} HEAD_MEAN worst |err| / (H 2^-24 |mean|) = {wm:.3f}")
    assert wm <= 1.0
    full2, _ = r.run(ar.FULL)
    assert torch.equal(full, full2)
    # lse + 0.5 scales every output by e^-0.5: the lse is used as given, not re-derived from the scores
    lse2 = lse + 0.5
    p2, bound2 = ar.probs_ref(q, k, lse2, dtype)
    assert float((p2 - p * torch.exp(-(lse2.double() - lse.double()))[..., None]).abs().max()) <= 1e-12
    shifted, _ = r.run(ar.FULL, lse=filled(lse2))
    assert ar.worst_ratio(shifted, p2, bound2) <= 1.0
    # and the two outputs stand in that ratio, as far as their two relative bounds r1, r2 allow
    want = torch.exp(-(lse2.double() - lse.double()))[..., None]
    r1, r2 = bound / p, bound2 / p2
    ratio = shifted.double() / full.double()
    assert bool((ratio >= want * (1 - r2) / (1 + r1)).all()) and bool((ratio <= want * (1 + r2) / (1 - r1)).all())
    assert abs(float(want.mean()) - np.exp(-0.5)) <= 1e-6          # 0.5 survives the fp32 addition to the lse


@pytest.mark.parametrize("dtype", DTYPES, ids=[ar.DT_NAME[d] for d in DTYPES])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_op_against_float64(hiplib, shape, dtype):
    check_op(hiplib, shape, dtype)


def test_op_real_size_bf16(hiplib):
    check_op(hiplib, REAL, ar.BF16)


@pytest.mark.parametrize("dtype", DTYPES, ids=[ar.DT_NAME[d] for d in DTYPES])
def test_op_rows_sum_to_one_with_the_forward_lse(hiplib, dtype):
    """lse from sgl_op_attn_fwd itself: sum_j p_ij = exp(lse_true - lse_fwd) up to the element bounds, and the forward's lse
    is within kernel_ref's 2^-20 (1 + |lse|) of the true one: the map and the forward kernel agree."""
    shape = (2, 4, 143, 16)
    B, H, N, dh = shape
    q, k, lse_true, _, _ = op_case(shape, dtype)
    r = OpRun(hiplib, shape, dtype, q, k, lse_true)
    tdt = ar.TORCH_DT[dtype]
    v = filled(ar.pad_heads(torch.randn(B, H, N, dh, generator=torch.Generator().manual_seed(5)).to(tdt), r.DP))
    o = ah.Arena(B * N * H * dh * (4 if tdt == torch.float32 else 2), 0xFF)     # token-major [B*N][H*dh]
    lse_fwd = ah.Arena(B * H * N * 4, 0xFF)
    st = hiplib.sgl_op_attn_fwd(dtype, r.q.ptr, r.k.ptr, v.ptr, o.ptr, lse_fwd.ptr, B, H, N, dh, r.DP, 0, ah.stream())
    assert st == ah.OK
    torch.cuda.synchronize()
    lf = lse_fwd.f32(B, H, N).cpu()
    assert float(((lf.double() - lse_true.double()).abs() / (2.0 ** -20 * (1 + lse_true.double().abs()))).max()) <= 1.0
    full, _ = r.run(ar.FULL, lse=lse_fwd)
    p, bound = ar.probs_ref(q, k, lf, dtype)
    assert ar.worst_ratio(full, p, bound) <= 1.0
    tol = bound.sum(-1) + torch.expm1(2.0 ** -20 * (1 + lse_true.double().abs()))
    dev = (full.double().sum(-1) - 1).abs()
    print(f"{ar.DT_NAME[dtype]} row sums: max |sum - 1| = {float(dev.max()):.3e}, worst / bound = {float((dev / tol).max()):.3f}")
    assert float((dev / tol).max()) <= 1.0


# ---------------------------------------------------------------------------------------------------------------
# encoder
# ---------------------------------------------------------------------------------------------------------------
def case_setup(pkg, name):
    meta, att = load_case(name)
    cfg = pkg.get_config(str(meta["meta.config"]))
    seed = int(meta["meta.seed"])
    sd = pkg.weights.seeded_state_dict(cfg, seed=seed)
    x = pkg.weights.seeded_pixels(int(meta["meta.batch"]), int(meta["meta.res_h"]), int(meta["meta.res_w"]), seed=seed + 1000)
    return meta, att, cfg, sd, x


def make_model(pkg, cfg, sd, mode):
    m = pkg.SiglipVisionModelHIP(cfg, compute_dtype=mode).to("cuda")
    m.load_state_dict(sd)
    return m


_ENC = {}


def enc_run(pkg, name, mode):
    """One grad-enabled output_attentions call per (case, mode), shared (CPU copies; never modified)."""
    if (name, mode) not in _ENC:
        meta, att, cfg, sd, x = case_setup(pkg, name)
        m = make_model(pkg, cfg, sd, mode)
        out = m(pixel_values=x.cuda(), output_hidden_states=True, interpolate_pos_encoding=True, output_attentions=True)
        torch.cuda.synchronize()
        _ENC[(name, mode)] = dict(att=[a.cpu() for a in out.attentions], pool=out.pooling_attention.cpu(),
                                  hs=[h.detach().cpu() for h in out.hidden_states], requires_grad=[
                                      a.requires_grad for a in out.attentions] + [out.pooling_attention.requires_grad])
    return _ENC[(name, mode)]


def l2rel(a, ref):
    return float((a.double() - ref.double()).norm() / ref.double().norm())


@pytest.mark.parametrize("mode", ENC_MODES)
@pytest.mark.parametrize("name", CASES)
def test_encoder_maps_against_hf(pkg, hiplib, name, mode):
    meta, att, cfg, sd, x = case_setup(pkg, name)
    got = enc_run(pkg, name, mode)
    pool_ref = torch.from_numpy(meta["pooling"])
    assert len(got["att"]) == len(att) and not any(got["requires_grad"])
    for l, (a, ref) in enumerate(zip(got["att"], att)):
        assert a.shape == ref.shape and a.dtype == torch.float32
        err, rel = float((a - ref).abs().max()), l2rel(a, ref)
        if mode in ("fp32", "bf16x3"):
            print(f"{name} {mode} layer {l}: max|err| {err:.3e} (l2rel {rel:.3e})")
            assert err <= 1e-3
        else:
            yard = float(meta[("bf16ac." if mode == "bf16" else "fp16ac.") + "attn.l2rel"][l])
            print(f"{name} {mode} layer {l}: l2rel {rel:.3e} = {rel / yard:.2f} x HF autocast ({yard:.3e})")
            assert rel <= 2 * yard
    assert got["pool"].shape == pool_ref.shape
    if mode in ("fp32", "bf16x3"):
        assert float((got["pool"] - pool_ref).abs().max()) <= 1e-3
    else:
        yard = float(meta[("bf16ac." if mode == "bf16" else "fp16ac.") + "pooling.l2rel"])
        rel = l2rel(got["pool"], pool_ref)
        print(f"{name} {mode} pooling: l2rel {rel:.3e} = {rel / yard:.2f} x HF autocast ({yard:.3e})")
        assert rel <= 2 * yard


@pytest.mark.parametrize("mode", ENC_MODES)
@pytest.mark.parametrize("name", CASES)
def test_encoder_rows_sum_to_one(pkg, hiplib, name, mode):
    """Row sums against the reference's bound.  The bound needs the magnitudes of the scores and of the lse, which the maps
    do not show (a common offset of a row's scores cancels in p): they are rebuilt in float64 from the block's input hidden
    state (an output of the same call) and the weights, and enter the bound only as magnitudes."""
    meta, att, cfg, sd, x = case_setup(pkg, name)
    got = enc_run(pkg, name, mode)
    Hh, D = cfg.num_attention_heads, cfg.hidden_size
    dh = D // Hh
    dtype = {"fp32": ar.F32, "bf16x3": ar.BF16X3, "bf16": ar.BF16, "fp16": ar.F16}[mode]
    for l, a in enumerate(got["att"]):
        h = got["hs"][l].double()
        pre = f"encoder.layers.{l}."
        h1 = torch.nn.functional.layer_norm(h, (D,), sd[pre + "layer_norm1.weight"].double(),
                                            sd[pre + "layer_norm1.bias"].double(), cfg.layer_norm_eps)
        heads = lambda t: t.view(t.shape[0], t.shape[1], Hh, dh).transpose(1, 2)
        q = heads(h1 @ sd[pre + "self_attn.q_proj.weight"].double().t() + sd[pre + "self_attn.q_proj.bias"].double())
        k = heads(h1 @ sd[pre + "self_attn.k_proj.weight"].double().t() + sd[pre + "self_attn.k_proj.bias"].double())
        lse = torch.logsumexp((q @ k.transpose(-1, -2)) * dh ** -0.5, -1)
        p, bound = ar.probs_ref(q, k, lse, dtype)
        tol = bound.sum(-1) + torch.expm1(2.0 ** -20 * (1 + lse.abs()))
        dev = (a.double().sum(-1) - 1).abs()
        print(f"{name} {mode} layer {l}: max |row sum - 1| = {float(dev.max()):.3e}, worst / bound {float((dev / tol).max()):.3f}")
        assert float((dev / tol).max()) <= 1.0
        assert float(a.min()) >= 0.0


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
@pytest.mark.parametrize("name", ["tiny_208x176", "hostile_59x101"])
def test_flag_changes_nothing_else(pkg, hiplib, name, mode):
    """no_grad gives the bits of the grad-enabled call; with the flag, every output and, after backward(), every gradient
    is bit-equal to a run without it."""
    meta, att, cfg, sd, x = case_setup(pkg, name)
    xg = x.cuda()
    taps = (1, cfg.num_hidden_layers)

    def run(flag, grad=True):
        m = make_model(pkg, cfg, sd, mode)
        kw = dict(output_attentions=True) if flag else {}
        with torch.enable_grad() if grad else torch.no_grad():
            out = m(pixel_values=xg, hidden_state_ids=taps, interpolate_pos_encoding=True, **kw)
        grads = None
        if grad:
            loss = out.pooler_output.square().sum() + out.last_hidden_state.square().mean() + \
                sum(h.square().mean() for h in out.hidden_states)
            loss.backward()
            grads = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
        torch.cuda.synchronize()
        return out, grads

    plain, g_plain = run(False)
    flagged, g_flag = run(True)
    quiet, _ = run(True, grad=False)
    infer, _ = run(False, grad=False)
    for other in (flagged, quiet, infer):
        assert torch.equal(other.pooler_output, plain.pooler_output)
        assert torch.equal(other.last_hidden_state, plain.last_hidden_state)
        for a, b in zip(other.hidden_states, plain.hidden_states):
            assert torch.equal(a, b)
    assert plain.attentions is None and plain.pooling_attention is None
    assert g_plain.keys() == g_flag.keys() and len(g_plain) > 0
    for n in g_plain:
        assert torch.equal(g_plain[n], g_flag[n]), n
    # the maps themselves: the same bits in both grad modes, and those of the shared run
    shared = enc_run(pkg, name, mode)
    for a, b, c in zip(flagged.attentions, quiet.attentions, shared["att"]):
        assert torch.equal(a, b) and torch.equal(a.cpu(), c)
        assert not a.requires_grad and not b.requires_grad
    assert torch.equal(flagged.pooling_attention, quiet.pooling_attention)


@pytest.mark.parametrize("mode", ["bf16", "bf16x3"])
def test_layer_subsets_mean_and_rollout(pkg, hiplib, mode):
    name = "tiny_208x176"
    meta, att, cfg, sd, x = case_setup(pkg, name)
    shared = enc_run(pkg, name, mode)
    m = make_model(pkg, cfg, sd, mode)
    xg = x.cuda()
    Hh = cfg.num_attention_heads
    with torch.no_grad():
        sub = m(pixel_values=xg, interpolate_pos_encoding=True, output_attentions=True, attention_layers=[2, 0, -1])
        assert len(sub.attentions) == 3
        for a, l in zip(sub.attentions, (2, 0, 2)):
            assert torch.equal(a.cpu(), shared["att"][l])
        with torch.inference_mode():
            inf = m(pixel_values=xg, interpolate_pos_encoding=True, output_attentions=True, attention_layers=[1])
        assert torch.equal(inf.attentions[0].cpu(), shared["att"][1])
        none = m(pixel_values=xg, interpolate_pos_encoding=True, output_attentions=True, attention_layers=[])
        assert none.attentions == () and torch.equal(none.pooling_attention.cpu(), shared["pool"])
        mean = m(pixel_values=xg, interpolate_pos_encoding=True, output_attentions=True, attention_heads="mean")
        assert len(mean.attentions) == cfg.num_hidden_layers
        for a, full in zip(mean.attentions, shared["att"]):
            assert a.shape == (full.shape[0], full.shape[2], full.shape[3])
            ref, bound = ar.head_mean_ref(full)
            assert ar.worst_ratio(a.cpu(), ref, bound) <= 1.0
        pm = shared["pool"].double().mean(1)
        assert mean.pooling_attention.shape == pm.shape
        assert float(((mean.pooling_attention.cpu().double() - pm).abs() / (Hh * ar.EPS32 * pm)).max()) <= 1.0
        roll = m.attention_rollout(xg, residual=0.5)
        P = cfg.patch_size
        assert roll.shape == (xg.shape[0], xg.shape[2] // P, xg.shape[3] // P) and not roll.requires_grad
        ref = pkg.heads.attention_rollout(mean.attentions, 0.5, pooling=mean.pooling_attention)
        assert torch.equal(roll.reshape(ref.shape), ref)
        # rows of every mixed matrix are renormalised and the probe map sums to 1: L + 1 fp32 N-term sums
        N = full.shape[-1]
        assert float((roll.double().sum((1, 2)) - 1).abs().max()) <= 2 * (len(shared["att"]) + 1) * (N + 8) * ar.EPS32


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_abi_arena_is_only_read(pkg, hiplib, mode):
    """sgl_attention_probs straight on the C ABI: every layer and the pooling head, both modes, into guarded outputs; the
    saved arena (every byte 0xFF = NaN before the forward) keeps its bits and its guards, and every output element is
    written with a finite value."""
    B, H, W = 2, 59, 101
    with ah.Session(pkg, hiplib, "hostile", mode) as ses:
        shadow = ses.new_shadow()
        assert ses.prepare(shadow, full=True) == ah.OK
        run = ah.Run(ses, B, H, W, train=True, fill=0xFF, kind="slots")
        assert ses.forward(run, shadow, ses.pixels(B, H, W), kind="slots") == ah.OK
        torch.cuda.synchronize()
        before = run.saved.payload.clone()
        N, Hh, L = run.N, ses.cfg.num_attention_heads, ses.Lyr
        for layer in range(L + 1):
            for md in (ar.FULL, ar.HEAD_MEAN):
                shape = ((B,) if md else (B, Hh)) + ((N,) if layer == L else (N, N))
                out = ah.Arena(int(np.prod(shape)) * 4, 0xFF)
                st = hiplib.sgl_attention_probs(ses.ctx, B, H, W, run.saved.ptr, run.saved.nbytes, layer, md, out.ptr,
                                                out.nbytes, ah.stream())
                assert st == ah.OK, (layer, md, st)
                torch.cuda.synchronize()
                assert out.guards_intact() and run.saved.guards_intact()
                t = out.f32(*shape)
                assert bool(torch.isfinite(t).all()) and float(t.min()) >= 0.0
        assert torch.equal(run.saved.payload, before)


def test_flag_under_torch_compile_is_a_graph_break(pkg, hiplib):
    """torch.compile of the model: the flagged call leaves the graph (``@torch.compiler.disable``) and returns the maps of
    the eager call; the unflagged call still compiles as it did."""
    name, mode = "tiny_48", "bf16"
    meta, att, cfg, sd, x = case_setup(pkg, name)
    shared = enc_run(pkg, name, mode)
    m = make_model(pkg, cfg, sd, mode)
    cm = torch.compile(m)
    xg = x.cuda()
    with torch.no_grad():
        eager = m(pixel_values=xg, interpolate_pos_encoding=True)
        out = cm(pixel_values=xg, interpolate_pos_encoding=True, output_attentions=True)
        plain = cm(pixel_values=xg, interpolate_pos_encoding=True)
    for a, b in zip(out.attentions, shared["att"]):
        assert torch.equal(a.cpu(), b)
    assert torch.equal(out.pooler_output, eager.pooler_output) and torch.equal(plain.pooler_output, eager.pooler_output)
    assert plain.attentions is None
