"""GPU: the block-recompute policy (model.recompute / sgl_create_ex(..., SGL_RECOMPUTE_BLOCKS)).

Recompute runs the forward's kernels on the same bits (the training path is bitwise reproducible), so everything it
produces (outputs, taps, every parameter gradient) must be BITWISE equal to the default policy's."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _model(pkg, name, mode, seed=3, recompute=False):
    cfg = pkg.get_config(name)
    m = pkg.SiglipVisionModelHIP(cfg, compute_dtype=mode, recompute=recompute)
    m.load_state_dict(pkg.weights.seeded_state_dict(cfg, seed=seed))
    return m.cuda()


def _weights_like(out, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return [torch.randn(t.shape, device="cuda", generator=g) for t in out]


def _step(model, x, taps=None, interp=True, seed=5):
    """Forward + backward with a loss on pooled, last and tap outputs; returns (outputs, {name: grad})."""
    for p in model.parameters():
        p.grad = None
    out = model(pixel_values=x, interpolate_pos_encoding=interp, hidden_state_ids=taps,
                output_hidden_states=taps is None)
    ts = [out.pooler_output, out.last_hidden_state] + list(out.hidden_states or ())
    ws = _weights_like(ts, seed)
    loss = sum((t * w).sum() for t, w in zip(ts, ws) if t.requires_grad)
    loss.backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    return [t.detach().clone() for t in ts], grads


def _assert_bitwise(a, b):
    (oa, ga), (ob, gb) = a, b
    assert len(oa) == len(ob)
    for i, (x, y) in enumerate(zip(oa, ob)):
        assert torch.equal(x, y), f"output {i}"
    assert ga.keys() == gb.keys() and ga
    for n in ga:
        assert torch.equal(ga[n], gb[n]), n


@pytest.mark.parametrize("mode", ["fp32", "bf16", "bf16x3", "fp16"])
@pytest.mark.parametrize("case", [("tiny", 2, 48, True), ("hostile", 2, 42, False)])
def test_recompute_is_bitwise_equal(pkg, hiplib, mode, case):
    name, B, res, interp = case
    model = _model(pkg, name, mode)
    x = pkg.weights.seeded_pixels(B, res, res, seed=11).cuda()
    taps = None if interp else [0, 1]
    ref = _step(model, x, taps, interp)
    model.recompute = True
    got = _step(model, x, taps, interp)
    _assert_bitwise(ref, got)


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
def test_recompute_is_bitwise_equal_full_width(pkg, hiplib, mode):
    """so400m block at 384 px: 256x256 GEMM tiles and the split-K dW path."""
    model = _model(pkg, "so400m-1layer", mode)
    x = pkg.weights.seeded_pixels(4, 384, 384, seed=2).cuda()
    ref = _step(model, x, [0, 1])
    model.recompute = True
    _assert_bitwise(ref, _step(model, x, [0, 1]))


def test_recompute_sid_frozen_prefix_channels_last(pkg, hiplib):
    """The SID shape: embeddings and blocks < 2 frozen, taps on frozen and trainable blocks, channels_last input; the
    first trainable block runs without an input gradient (need_dx = 0) and frozen blocks are never recomputed."""
    model = _model(pkg, "tiny", "bf16")
    for p in model.embeddings.parameters():
        p.requires_grad_(False)
    for i, lyr in enumerate(model.encoder.layers):
        for p in lyr.parameters():
            p.requires_grad_(i >= 2)
    x = pkg.weights.seeded_pixels(3, 48, 48, seed=4).cuda().contiguous(memory_format=torch.channels_last)
    ref = _step(model, x, [1, 2, 3])
    model.recompute = True
    got = _step(model, x, [1, 2, 3])
    _assert_bitwise(ref, got)
    assert "encoder.layers.2.mlp.fc1.weight" in got[1] and "encoder.layers.1.mlp.fc1.weight" not in got[1]


def test_policy_change_between_forward_and_backward(pkg, hiplib):
    """A backward runs with its forward's policy; two calls with different policies may share one loss."""
    model = _model(pkg, "hostile", "bf16")
    x = pkg.weights.seeded_pixels(2, 42, 42, seed=8).cuda()
    ref = _step(model, x, [1])
    for first in (False, True):
        model.recompute = first
        for p in model.parameters():
            p.grad = None
        out = model(pixel_values=x, hidden_state_ids=[1])
        model.recompute = not first
        ts = [out.pooler_output, out.last_hidden_state, out.hidden_states[0]]
        sum((t * w).sum() for t, w in zip(ts, _weights_like(ts, 5))).backward()
        torch.cuda.synchronize()
        _assert_bitwise(ref, ([t.detach() for t in ts], {n: p.grad.clone() for n, p in model.named_parameters()}))
    # two encoder calls, one per policy, in one loss: gradients add up to twice the single-call gradients
    x2 = pkg.weights.seeded_pixels(2, 42, 42, seed=9).cuda()
    model.recompute = False
    r1 = _step(model, x, [1])
    r2 = _step(model, x2, [1], seed=6)
    for p in model.parameters():
        p.grad = None
    model.recompute = False
    oa = model(pixel_values=x, hidden_state_ids=[1])
    model.recompute = True
    ob = model(pixel_values=x2, hidden_state_ids=[1])
    ta = [oa.pooler_output, oa.last_hidden_state, oa.hidden_states[0]]
    tb = [ob.pooler_output, ob.last_hidden_state, ob.hidden_states[0]]
    la = sum((t * w).sum() for t, w in zip(ta, _weights_like(ta, 5)))
    lb = sum((t * w).sum() for t, w in zip(tb, _weights_like(tb, 6)))
    (la + lb).backward()
    torch.cuda.synchronize()
    for i in range(3):
        assert torch.equal(ta[i].detach(), r1[0][i]) and torch.equal(tb[i].detach(), r2[0][i])
    for n, p in model.named_parameters():
        assert torch.equal(p.grad, r1[1][n] + r2[1][n]), n


def test_fused_adamw_steps_with_recompute(pkg, hiplib):
    res = {}
    for rc in (False, True):
        model = _model(pkg, "hostile", "bf16", recompute=rc)
        opt = pkg.FusedAdamW(model.parameters(), lr=1e-3, weight_decay=0.01, max_grad_norm=0.5)
        losses = []
        for step in range(3):
            x = pkg.weights.seeded_pixels(2, 42, 42, seed=20 + step).cuda()
            opt.zero_grad(set_to_none=True)
            out = model(pixel_values=x, hidden_state_ids=[1])
            loss = out.pooler_output.square().mean() + out.last_hidden_state.mean() + out.hidden_states[0].square().mean()
            loss.backward()
            opt.step()
            losses.append(loss.detach().clone())
        torch.cuda.synchronize()
        res[rc] = (losses, [p.detach().clone() for p in model.parameters()])
    for a, b in zip(res[False][0], res[True][0]):
        assert torch.equal(a, b)
    for a, b in zip(res[False][1], res[True][1]):
        assert torch.equal(a, b)


def test_torch_compile_with_recompute(pkg, hiplib):
    cfg = pkg.get_config("hostile")
    enc = pkg.OpenClipStyleEncoder(cfg, "bf16")
    enc.visual.load_state_dict(pkg.weights.seeded_state_dict(cfg, 0))
    enc.set_grad_checkpointing(True)
    model = pkg.heads.FastBinaryClassifierHIP(enc, "small").cuda().eval()
    x = pkg.weights.seeded_pixels(4, 42, 42, seed=1).cuda()
    ref = model(x)
    ref.sum().backward()
    g0 = {n: p.grad.clone() for n, p in model.backbone.visual.named_parameters()}
    for p in model.parameters():
        p.grad = None
    out = torch.compile(model, fullgraph=True)(x)
    out.sum().backward()
    assert torch.allclose(out, ref, atol=1e-5)     # the compiled head may round differently from eager
    for n, p in model.backbone.visual.named_parameters():
        assert p.grad is not None, n
        assert ((p.grad - g0[n]).norm() / g0[n].norm().clamp_min(1e-30)).item() <= 1e-3, n
    # the encoder call alone under torch.compile: bitwise eager
    vis = enc.visual
    f = torch.compile(lambda t: vis(pixel_values=t, hidden_state_ids=[1]), fullgraph=True)
    ref = _step(vis, x, [1], interp=False)
    for p in vis.parameters():
        p.grad = None
    o = f(x)
    ts = [o.pooler_output, o.last_hidden_state, o.hidden_states[0]]
    sum((t * w).sum() for t, w in zip(ts, _weights_like(ts, 5))).backward()
    _assert_bitwise(ref, ([t.detach() for t in ts], {n: p.grad.clone() for n, p in vis.named_parameters()}))


def test_recompute_memory_so400m(pkg, hiplib):
    """Bytes held from forward to backward (saved + hidden states) at so400m@384, B = 8: with its shared block region
    counted in, recompute holds at most 0.2x of the default; both agree with the size query within 1 %."""
    B, N, D, L = 8, 729, 1152, 27
    x = pkg.weights.seeded_pixels(B, 384, 384, seed=3).cuda()
    held = {}
    for rc in (False, True):
        model = _model(pkg, "so400m-patch14-384", "bf16", recompute=rc)
        for _ in range(2):       # the first step allocates the workspace cache; measure the second
            for p in model.parameters():
                p.grad = None
            torch.cuda.synchronize()
            before = torch.cuda.memory_allocated()
            out = model(pixel_values=x)
            torch.cuda.synchronize()
            after = torch.cuda.memory_allocated()
            (out.pooler_output.sum() + out.last_hidden_state.mean()).backward()
            del out
        # outputs: last_hidden_state and pooled are not part of the held activations
        held[rc] = after - before - B * N * D * 4 - B * D * 4
        sizes = model._contexts.sizes(B, 384, 384, True, rc)
        predicted = sizes[1] + (L + 1) * B * N * D * 4
        assert abs(held[rc] - predicted) <= 0.01 * predicted, (rc, held[rc], predicted)
        if rc:
            region = sizes[2] - model._contexts.sizes(B, 384, 384, True, False)[2]
        del model
        torch.cuda.empty_cache()
    assert held[True] + region <= 0.2 * held[False], (held, region)


def test_recompute_large_token_count(pkg, hiplib):
    """so400m block at the recompute context's token limit (u / a / du above 2^31 bytes): the first and last images match
    a B = 4 run on the same images, and the parameter gradients match those accumulated over 4 chunks."""
    m = _model(pkg, "so400m-1layer", "bf16", recompute=True)
    N = 729
    B = 700
    while _query(pkg, m, B) != 0:      # the enforced training token limit, when it is below B = 700
        B -= 1
    assert B >= 600 and B * N * 4352 * 2 > 2 ** 31
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.rand(B, 3, 384, 384, device="cuda", generator=g) * 2 - 1
    wl = torch.randn(B, N, 1152, device="cuda", generator=g)
    wp = torch.randn(B, 1152, device="cuda", generator=g)

    def run(lo, hi):
        out = m(pixel_values=x[lo:hi])
        ((out.last_hidden_state * wl[lo:hi]).sum() + (out.pooler_output * wp[lo:hi]).sum()).backward()
        return out.last_hidden_state.detach()

    last = run(0, B)
    first_last = (last[0].clone(), last[-1].clone())
    del last
    full = {n: p.grad.clone() for n, p in m.named_parameters()}
    for p in m.parameters():
        p.grad = None
    small = m(pixel_values=torch.cat([x[:2], x[-2:]])).last_hidden_state.detach()
    for got, ref in ((first_last[0], small[0]), (first_last[1], small[-1])):
        assert ((got - ref).norm() / ref.norm()).item() <= 1e-5
    for p in m.parameters():
        p.grad = None
    cuts = [0, B // 4, B // 2, 3 * B // 4, B]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        run(lo, hi)                                  # gradients accumulate into .grad
    torch.cuda.synchronize()
    for n, p in m.named_parameters():
        rel = ((p.grad - full[n]).norm() / full[n].norm().clamp_min(1e-30)).item()
        assert rel <= 1e-4, (n, rel)


def _query(pkg, m, B):
    return pkg.lib.load().sgl_query_sizes(m._contexts.get(True), B, 384, 384, 1, None, None, None)
