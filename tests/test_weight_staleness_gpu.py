"""GPU: every route that writes weights against every cached copy of them.

The project keeps derived copies of the fp32 master parameters ("Derived copies of the weights"): the encoder's
shadow arena (``encoder_state.WeightShadows``, keyed on ``(data_ptr, _version)`` per parameter), the decoder's bf16 weight
cache (``head_ops.WeightCache``, ``(_version, data_ptr)``), ``FusedAdamW``'s device tables with the shadow destinations
bound into them, and the ``ExponentialMovingAverage`` plan (both keyed on pointers).  Each is right only while every write
moves its key.

The oracle is a FRESH TWIN: a new model object built from a clone of the written model's ``state_dict()`` that has never
run (no arena, no cache entry, no optimizer table), given the same input and the same upstream gradients.  Outputs, taps
and every gradient must be ``torch.equal``: the reductions have a fixed order, so there is no tolerance.  Two controls are
asserted with it: two fresh twins agree bit for bit (determinism), and the write changed what is compared (sensitivity).
"""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

TRAIN_MODES = ["fp32", "bf16x3", "bf16", "fp16"]
# parameters a write of which cancels in the forward (softmax is invariant to a per-query shift of the scores): the
# sensitivity control is then made on outputs AND gradients together
KEY_BIAS = ("self_attn.k_proj.bias",)


# ---------------------------------------------------------------------------------------------------------
# building, running, comparing
# ---------------------------------------------------------------------------------------------------------
def _cosw(t, phase):
    idx = torch.arange(t.numel(), dtype=torch.float32, device=t.device).reshape(t.shape)
    return torch.cos(idx * 0.37 + phase)


def _delta(p, k):
    """A deterministic perturbation with the parameter's shape and device, about 0.05 large."""
    idx = torch.arange(p.numel(), dtype=torch.float32, device=p.device)
    return (0.05 * torch.cos(idx * 0.7 + 0.3 * k) + 0.02).reshape(p.shape)


def make_encoder(pkg, cfg_name, mode, seed=5, recompute=False):
    cfg = pkg.get_config(cfg_name)
    model = pkg.SiglipVisionModelHIP(cfg, compute_dtype=mode, recompute=recompute)
    model.load_state_dict(pkg.weights.seeded_state_dict(cfg, seed=seed))
    return model.cuda()


def make_decoder(pkg, seed=0):
    torch.manual_seed(seed)
    return pkg.heads.SegFormerMaskDecoder([16, 16], embed_dim=8).cuda()


def fresh_twin(model):
    """A new object of the model's class from a clone of its state_dict: same values, same requires_grad, never run."""
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    twin = _blank_like(model).cuda()
    twin.load_state_dict(sd)
    for a, b in zip(twin.parameters(), model.parameters()):
        a.requires_grad = b.requires_grad
    return twin.train(model.training)


def _blank_like(model):
    import __graft_entry__ as entry
    pkg = entry.load_package()
    if isinstance(model, pkg.SiglipVisionModelHIP):
        return type(model)(model.config, model.compute_dtype, model.recompute)
    if isinstance(model, pkg.heads.SegFormerMaskDecoder):
        return pkg.heads.SegFormerMaskDecoder([16, 16], embed_dim=8)
    if isinstance(model, pkg.heads.ImageBinaryClassifierHIP):
        vis = model.backbone.visual
        return pkg.heads.ImageBinaryClassifierHIP(pkg.OpenClipStyleEncoder(vis.config, vis.compute_dtype))
    if isinstance(model, torch.nn.ModuleDict):
        return torch.nn.ModuleDict({k: _blank_like(v) for k, v in model.items()})
    raise TypeError(type(model))


def encoder_pixels(pkg, model, batch=2):
    res = model.config.image_size
    return pkg.weights.seeded_pixels(batch, res, res, seed=8).cuda()


def run_encoder_infer(model, x):
    with torch.no_grad():
        out = model(pixel_values=x, output_hidden_states=True)
    res = {"infer.last": out.last_hidden_state.clone()}
    if out.pooler_output is not None:
        res["infer.pooled"] = out.pooler_output.clone()
    for i, h in enumerate(out.hidden_states):
        res[f"infer.hs{i}"] = h.clone()
    return res


def run_encoder_train(model, x):
    """Training forward with every tap, backward from a fixed weighting of pooled / last / taps."""
    model.zero_grad(set_to_none=True)
    out = model(pixel_values=x, output_hidden_states=True)
    loss = (out.pooler_output * _cosw(out.pooler_output, 0.11)).sum() + \
        0.1 * (out.last_hidden_state * _cosw(out.last_hidden_state, 0.5)).sum()
    for i, h in enumerate(out.hidden_states):
        loss = loss + 0.05 * (h * _cosw(h, 0.2 * i)).sum()
    loss.backward()
    res = {"train.pooled": out.pooler_output.detach().clone(), "train.last": out.last_hidden_state.detach().clone()}
    for i, h in enumerate(out.hidden_states):
        res[f"train.hs{i}"] = h.detach().clone()
    for n, p in model.named_parameters():
        if p.requires_grad:
            assert p.grad is not None, n
            res["grad." + n] = p.grad.detach().clone()
    return res


def _hip_linear_nodes(root):
    """Every _HipLinearFnBackward node below ``root``, in a fixed (depth-first) order."""
    seen, order, stack = set(), [], [root]
    while stack:
        node = stack.pop()
        if node is None or node in seen:
            continue
        seen.add(node)
        if type(node).__name__ == "_HipLinearFnBackward":
            order.append(node)
        stack.extend(fn for fn, _ in reversed(node.next_functions))
    return order


DEC_HIP_LINEARS = 7    # 2 tap projections, 2 smoothing 1x1, gate squeeze (K = 16), fuse, mask head; the gate's K = 4 is F.linear


def decoder_taps():
    g = torch.Generator().manual_seed(21)
    return [torch.randn(1, 64, 16, generator=g).cuda() for _ in range(2)]


def run_decoder(dec, taps):
    """Forward and backward under bf16 autocast on (1, 64, 16) taps, grid 8 x 8: 64 rows, K % 8 == 0, the smallest case
    ``linear_tokens`` sends to the HIP GEMM.  Returns the logits, every parameter gradient, the tap gradients and the dX
    each HIP linear's backward produced (the GEMM that reads the cached transpose)."""
    dec.zero_grad(set_to_none=True)
    taps = [t.detach().clone().requires_grad_(True) for t in taps]
    with torch.autocast("cuda", dtype=torch.bfloat16):
        logit = dec(taps, (8, 8), return_lowres=True)
    nodes = _hip_linear_nodes(logit.grad_fn)
    assert len(nodes) == DEC_HIP_LINEARS, f"{len(nodes)} HIP linear nodes: the decoder fell back to F.linear"
    dxs = {}
    for i, node in enumerate(nodes):
        node.register_hook(lambda gin, gout, i=i: dxs.__setitem__(i, gin[0].detach().clone()))
    logit.backward(_cosw(logit, 0.4).to(logit.dtype))
    res = {"dec.logit": logit.detach().clone()}
    assert len(dxs) == DEC_HIP_LINEARS
    for i in range(DEC_HIP_LINEARS):
        res[f"dec.dx{i}"] = dxs[i]
    for i, t in enumerate(taps):
        res[f"dec.dtap{i}"] = t.grad.clone()
    for n, p in dec.named_parameters():
        res["dec.grad." + n] = p.grad.detach().clone()
    return res


def differing(a, b):
    assert a.keys() == b.keys(), sorted(set(a) ^ set(b))
    return [k for k in a if a[k].shape != b[k].shape or not torch.equal(a[k], b[k])]


def assert_same(got, want, what):
    bad = differing(got, want)
    assert not bad, f"{what}: {len(bad)} of {len(got)} tensors differ from the fresh twin's, e.g. {bad[:6]}"


def assert_changed(got, prev, what, prefixes):
    """Sensitivity control: in every consumer (key prefix) the write changed something that is compared."""
    bad = set(differing(got, prev))
    for pre in prefixes:
        assert any(k.startswith(pre) for k in bad), f"{what}: the write changed nothing under '{pre}' (vacuous case)"


def write_all(module, k=0):
    with torch.no_grad():
        for i, p in enumerate(module.parameters()):
            p.add_(_delta(p, k + i))


# ---------------------------------------------------------------------------------------------------------
# A. every field of the parameter table, every compute mode
# ---------------------------------------------------------------------------------------------------------
def _field_matrix(pkg, cfg_name, mode, recompute=False, train=True):
    model = make_encoder(pkg, cfg_name, mode, recompute=recompute)
    x = encoder_pixels(pkg, model)
    if not train:
        model.requires_grad_(False)
    run = (lambda m: {**run_encoder_train(m, x), **run_encoder_infer(m, x)}) if train else \
        (lambda m: run_encoder_infer(m, x))
    # determinism control: two fresh twins agree bit for bit in this mode
    t1, t2 = fresh_twin(model), fresh_twin(model)
    assert_same(run(t1), run(t2), f"{cfg_name}/{mode}: two fresh twins")
    del t1, t2
    prev = run(model)       # warm: the arena, the transposes and (training) the saved state exist
    serial = model._shadows.serial
    entries = model._table.entries
    assert {e.unit for e in entries} == set(range(model.config.num_hidden_layers + 1))
    cases = 0
    for k, (e, p) in enumerate(zip(entries, model._table.params())):
        what = f"{cfg_name}/{mode}{'/recompute' if recompute else ''}: write of {e.path}"
        with torch.no_grad():
            p.add_(_delta(p, k))
        got = run(model)
        assert model._shadows.serial > serial, f"{what}: no unit was refreshed"
        serial = model._shadows.serial
        if e.path.endswith(KEY_BIAS):
            assert differing(got, prev), f"{what}: changed neither an output nor a gradient"
        else:
            assert_changed(got, prev, what, ["train.", "infer."] if train else ["infer."])
        assert_same(got, run(fresh_twin(model)), what)
        prev = got
        cases += 1
    assert cases == len(entries) == 3 + 16 * model.config.num_hidden_layers + 2 + 11
    print(f"[field matrix] {cfg_name}/{mode}{'/recompute' if recompute else ''}: {cases} fields, all equal to the twin")


@pytest.mark.parametrize("cfg_name,mode", [("tiny", m) for m in TRAIN_MODES] + [("hostile", "bf16"), ("hostile", "bf16x3")])
def test_every_field_write_reaches_forward_and_backward(pkg, hiplib, cfg_name, mode):
    """Every entry of the ParamTable (every block, and the global unit: patch weight and bias, position table, final
    LayerNorm, pooling head), written alone with ``p.add_`` after a warm forward + backward: training forward, backward and
    inference forward equal the fresh twin's.  Catches a field missing from the unit keys, a shadow (cast, transpose, split
    plane) that the dirty refresh does not remake, and anything only the backward reads."""
    _field_matrix(pkg, cfg_name, mode)


def test_every_field_write_reaches_the_recompute_backward(pkg, hiplib):
    _field_matrix(pkg, "tiny", "bf16", recompute=True)


@pytest.mark.parametrize("cfg_name", ["tiny", "hostile"])
def test_every_field_write_reaches_the_mxfp8_forward(pkg, hiplib, cfg_name):
    """mxfp8 is inference-only: the forward alone, on the MX-fp8 copies of the block weights."""
    _field_matrix(pkg, cfg_name, "mxfp8", train=False)


# ---------------------------------------------------------------------------------------------------------
# B. every write route, every consumer
# ---------------------------------------------------------------------------------------------------------
class Rig:
    """A warm encoder (tiny, bf16) and a warm stand-alone decoder under one ModuleDict, the consumers that read their
    derived weights (encoder inference forward, encoder training forward + backward, decoder forward + backward under bf16
    autocast with the dX of every linear), and the twin comparison after a write."""

    CONSUMERS = ["infer.", "train.", "grad.", "dec.logit", "dec.dx", "dec.grad."]

    def __init__(self, pkg, mode="bf16", cfg_name="tiny"):
        self.pkg = pkg
        self.both = torch.nn.ModuleDict({"enc": make_encoder(pkg, cfg_name, mode), "dec": make_decoder(pkg)})
        self.x = encoder_pixels(pkg, self.both["enc"])
        self.taps = decoder_taps()
        t1, t2 = fresh_twin(self.both), fresh_twin(self.both)
        first = self.run(t1)
        assert_same(first, self.run(t2), "two fresh twins")                 # determinism control
        self.twin = t1
        self.prev = self.run(self.both)                                     # warm
        assert_same(self.prev, first, "the model against its first twin")
        assert self.both["enc"]._shadows.arena is not None
        entries = self._cache_entries()
        assert len(entries) == DEC_HIP_LINEARS and all(e[2] is not None for e in entries), "warm cache: every transpose"

    def _cache_entries(self):
        cache = self.pkg.head_ops._weights._entries
        return [cache[p] for p in self.both["dec"].parameters() if p in cache]

    def run(self, both, train=True):
        res = run_encoder_infer(both["enc"], self.x)
        if train:
            res.update(run_encoder_train(both["enc"], self.x))
            res.update(run_decoder(both["dec"], self.taps))
        return res

    def verify(self, what, changed=True, unchanged=False, train=True):
        """Run every consumer on the written model and on a fresh twin: equal bit for bit.  changed: the results differ
        from the previous verify's in every consumer (sensitivity); unchanged: they equal them (a route that moves
        pointers or layouts without writing values)."""
        got = self.run(self.both, train)
        prev = {k: v for k, v in self.prev.items() if k in got}
        shared = {k: v for k, v in got.items() if k in prev}
        assert any(k.startswith("infer.") for k in shared)
        if unchanged:
            assert_same(shared, prev, f"{what}: against the same weights before")
        elif changed:
            assert_changed(shared, prev, what, [c for c in self.CONSUMERS if any(k.startswith(c) for k in shared)])
        self.twin = fresh_twin(self.both)
        assert_same(got, self.run(self.twin, train), what)
        self.prev = got
        return got

    def params(self, both=None):
        return [p for p in (self.both if both is None else both).parameters() if p.requires_grad]

    def step_and_verify(self, opt, make_opt, what):
        """One optimizer step on the model and on the twin of the last verify (which holds the same gradients), the twin's
        optimizer carrying a clone of the model's optimizer state: equal parameters after it, then every consumer again."""
        twin = self.twin
        for a, b in zip(self.params(), self.params(twin)):
            assert torch.equal(a.grad, b.grad)
        topt = make_opt(self.params(twin))
        if opt.state_dict()["state"]:
            topt.load_state_dict(copy.deepcopy(opt.state_dict()))
        opt.step()
        topt.step()
        for (n, a), (_, b) in zip(self.both.named_parameters(), twin.named_parameters()):
            assert torch.equal(a.detach(), b.detach()), f"{what}: {n} differs from the twin's after the step"
        return self.verify(what + ", consumers after the step")


def _fused(pkg, clip=0.7):
    return lambda params: pkg.FusedAdamW(params, lr=2e-2, weight_decay=0.05, max_grad_norm=clip)


def test_route_torch_adamw_step(pkg, hiplib):
    rig = Rig(pkg)
    make = lambda params: torch.optim.AdamW(params, lr=2e-2, weight_decay=0.05)
    opt = make(rig.params())
    for step in range(2):
        rig.step_and_verify(opt, make, f"torch.optim.AdamW step {step}")


def test_route_fused_adamw_step_without_attached_encoder(pkg, hiplib):
    rig = Rig(pkg)
    opt = _fused(pkg)(rig.params())
    for step in range(2):
        rig.step_and_verify(opt, _fused(pkg), f"FusedAdamW step {step}")


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_route_fused_adamw_step_writing_shadows_and_ema(pkg, hiplib, mode):
    """attach_encoder + attach_ema: the step writes the shadows itself and the next forward adopts them.  Three steps: the
    first binds the shadow destinations, the later ones reuse the device tables."""
    rig = Rig(pkg, mode)
    enc = rig.both["enc"]
    opt = _fused(pkg)(rig.params())
    opt.attach_encoder(enc)
    opt.attach_ema(pkg.ExponentialMovingAverage(rig.both, decay=0.5))
    for step in range(3):
        serial = enc._shadows.serial
        rig.step_and_verify(opt, _fused(pkg), f"FusedAdamW+encoder+EMA ({mode}) step {step}")
        assert enc._shadows.serial == serial + 1, "the step's shadows were adopted: no forward re-cast anything"


def test_route_load_state_dict(pkg, hiplib):
    rig = Rig(pkg)
    sd = {k: (v * 1.03 + 0.01 if v.is_floating_point() else v) for k, v in rig.both.state_dict().items()}
    rig.both.load_state_dict(sd)
    rig.verify("load_state_dict of different values")


def test_route_broadcast_write_back(pkg, hiplib):
    """``ddp.write_flat`` is the write primitive of ``broadcast_parameters`` (tests/test_ddp_gloo.py runs the two-rank
    collective on the CPU): after a warm forward it must leave no derived copy behind."""
    rig = Rig(pkg)
    tensors = [*rig.both.parameters(), *rig.both.buffers()]
    versions = [t._version for t in tensors]
    flat = torch.cat([t.detach().reshape(-1) for t in tensors])
    pkg.ddp.write_flat(tensors, flat * 0.95 + 0.01 * torch.cos(torch.arange(flat.numel(), device="cuda") * 0.3))
    assert all(t._version > v for t, v in zip(tensors, versions))
    rig.verify("broadcast write-back")


@pytest.mark.parametrize("forward_between", [True, False])
def test_route_ema_swap_and_restore(pkg, hiplib, forward_between):
    """apply_shadow -> (eval) -> restore -> train step, with FusedAdamW writing the encoder's shadows and the averages: the
    swap moves every data_ptr, so the arena, the weights struct, the decoder cache and the optimizer's device tables (which
    hold p.data_ptr()) are all rebuilt, twice."""
    rig = Rig(pkg)
    enc = rig.both["enc"]
    ema = pkg.ExponentialMovingAverage(rig.both, decay=0.5)
    opt = _fused(pkg)(rig.params())
    opt.attach_encoder(enc)
    opt.attach_ema(ema)
    rig.step_and_verify(opt, _fused(pkg), "step before the swap")          # the averages now differ from the weights
    before = rig.prev
    live_ptrs = [p.data_ptr() for p in rig.both.parameters()]
    ema.apply_shadow()
    assert all(p.data_ptr() != q for p, q in zip(rig.both.parameters(), live_ptrs))
    if forward_between:
        got = rig.verify("eval on the averages", train=False)
        for n, p in rig.both.named_parameters():
            assert torch.equal(p.detach(), ema.shadow[n]), n
        assert differing(got, {k: before[k] for k in got})
    ema.restore()
    assert [p.data_ptr() for p in rig.both.parameters()] == live_ptrs
    rig.prev = before
    rig.verify("training pass after restore", unchanged=True)              # the live weights were not written
    rig.step_and_verify(opt, _fused(pkg), "step after restore")
    rig.step_and_verify(opt, _fused(pkg), "second step after restore")


def test_route_ema_standalone_update_between_two_swaps(pkg, hiplib):
    """apply_shadow -> eval -> restore -> ema.update() with no parameter step -> apply_shadow -> eval.  The averages live
    at fixed addresses and ``update()`` does not touch the parameters: unless the swap itself moves the versions, the second
    eval shows the key of the first one to both caches while the averages have changed."""
    rig = Rig(pkg)
    ema = pkg.ExponentialMovingAverage(rig.both, decay=0.5)
    write_all(rig.both)                       # the weights leave the averages behind
    rig.verify("in-place write of everything")
    ema.update()
    ema.apply_shadow()
    keys = [(p.data_ptr(), p._version) for p in rig.both.parameters()]
    first = rig.verify("first eval on the averages")
    avg1 = {n: s.clone() for n, s in ema.shadow.items()}
    ema.restore()
    ema.update()
    assert all(not torch.equal(avg1[n], s) for n, s in ema.shadow.items())
    ema.apply_shadow()
    assert [p.data_ptr() for p in rig.both.parameters()] == [k[0] for k in keys]      # the same addresses again
    second = rig.verify("second eval, after a stand-alone update()")
    assert differing(first, second)
    ema.restore()
    rig.verify("training pass after the second restore")


def test_route_channels_last_after_a_forward(pkg, hiplib):
    """model.to(memory_format=torch.channels_last) re-lays the 4-D weights (the patch convolution, the decoder's
    convolutions) out at new addresses without changing a value; then a write and a FusedAdamW step on those layouts (no
    clipping: the global norm sums in storage order, which differs between the layouts of the model and of its twin)."""
    rig = Rig(pkg)
    enc = rig.both["enc"]
    rig.both.to(memory_format=torch.channels_last)
    pw = enc.embeddings.patch_embedding.weight
    assert not pw.is_contiguous() and pw.is_contiguous(memory_format=torch.channels_last)
    assert enc._shadows.arena is None, "nn.Module._apply releases the arena"
    rig.verify("after .to(channels_last)", unchanged=True)
    write_all(rig.both, 3)
    rig.verify("in-place write on channels_last layouts")
    opt = _fused(pkg, clip=None)(rig.params())
    opt.attach_encoder(enc)
    for step in range(2):
        rig.step_and_verify(opt, _fused(pkg, clip=None), f"FusedAdamW step {step} on channels_last layouts")


def test_route_deepcopy_of_a_warm_model(pkg, hiplib):
    """The copy shares no arena and inherits no cache entry; the original keeps its own."""
    rig = Rig(pkg)
    orig, orig_prev = rig.both, rig.prev
    clone = copy.deepcopy(orig)
    assert clone["enc"]._shadows is not orig["enc"]._shadows and clone["enc"]._shadows.arena is None
    cache = pkg.head_ops._weights._entries
    assert not any(p in cache for p in clone["dec"].parameters())
    write_all(clone, 5)
    rig.both = clone
    rig.verify("in-place write of a deepcopy")
    assert clone["enc"]._shadows.arena.data_ptr() != orig["enc"]._shadows.arena.data_ptr()
    rig.both, rig.prev = orig, orig_prev
    rig.verify("the original after its copy was written and run", unchanged=True)


def test_route_partially_unfreeze_backbone(pkg, hiplib):
    """A forward with the whole backbone frozen runs the encoder as inference; ``partially_unfreeze_backbone`` then turns
    the last block and every norm trainable: the next pass is a training forward from the first trainable block on, over
    the same arena."""
    H = pkg.heads
    cfg = pkg.get_config("tiny")
    bb = pkg.OpenClipStyleEncoder(cfg, "bf16")
    bb.visual.load_state_dict(pkg.weights.seeded_state_dict(cfg, 5))
    torch.manual_seed(1)
    clf = H.ImageBinaryClassifierHIP(bb).cuda().eval()          # eval: no dropout noise in a bitwise comparison
    x = encoder_pixels(pkg, bb.visual, batch=3)

    def run(m):
        m.zero_grad(set_to_none=True)
        logits = m(x)
        logits.backward(_cosw(logits, 0.3))
        res = {"logits": logits.detach().clone()}
        for n, p in m.named_parameters():
            if p.requires_grad:
                assert p.grad is not None, n
                res["grad." + n] = p.grad.detach().clone()
        return res

    assert_same(run(fresh_twin(clf)), run(fresh_twin(clf)), "two fresh twins")
    bb.requires_grad_(False)
    frozen = run(clf)
    assert bb.visual._shadows.arena is not None and not any(k.startswith("grad.backbone") for k in frozen)
    assert clf.partially_unfreeze_backbone(last_blocks=1) > 0
    got = run(clf)
    trainable = [k for k in got if k.startswith("grad.backbone")]
    assert any("layers.2.mlp" in k for k in trainable) and not any("layers.0.mlp" in k for k in trainable)
    assert torch.equal(got["logits"], frozen["logits"])
    assert_same(got, run(fresh_twin(clf)), "after partially_unfreeze_backbone")
    for k, layer in enumerate((bb.visual.encoder.layers[0], bb.visual.encoder.layers[2])):
        with torch.no_grad():                                   # a frozen block's weight, then a trainable block's
            layer.mlp.fc1.weight.add_(_delta(layer.mlp.fc1.weight, k))
        after = run(clf)
        assert differing(after, got)
        assert_same(after, run(fresh_twin(clf)), f"write of block {2 * k} after the unfreeze")
        got = after


# ---------------------------------------------------------------------------------------------------------
# C. writes between a forward and its backward
# ---------------------------------------------------------------------------------------------------------
def _train_forward(model, x):
    out = model(pixel_values=x)
    return (out.pooler_output * _cosw(out.pooler_output, 0.11)).sum()


def test_encoder_backward_refuses_shadows_recast_since_its_forward(pkg, hiplib):
    """The backward reads the arena its forward read.  Parameters changed + another forward in between = the arena holds
    other weights: the first forward's backward must raise and name the cause, never run on them.  An in-place write is
    caught first by autograd (the parameters are saved tensors); a ``.data`` swap (the reference's EMA helper), which
    autograd cannot see, reaches ``WeightShadows.check_backward``.  With nothing in between the backward runs."""
    model = make_encoder(pkg, "tiny", "bf16")
    x = encoder_pixels(pkg, model)
    fc1 = model.encoder.layers[1].mlp.fc1.weight

    loss = _train_forward(model, x)
    with torch.no_grad():
        model(pixel_values=x)                # a forward in between that re-casts nothing
    loss.backward()                          # must not raise
    want = fc1.grad.clone()

    # .data swap and back around an eval forward: versions stay, the arena was re-cast for the other weights
    loss = _train_forward(model, x)
    live = fc1.data
    fc1.data = live * 1.5
    with torch.no_grad():
        model(pixel_values=x)
    fc1.data = live
    with pytest.raises(RuntimeError, match="parameters changed between this forward and its backward"):
        loss.backward()

    # in-place write, then another forward
    loss = _train_forward(model, x)
    orig = fc1.detach().clone()
    with torch.no_grad():
        fc1.add_(0.01)
        model(pixel_values=x)
    with pytest.raises(RuntimeError, match="parameters changed between this forward and its backward|"
                                           "modified by an inplace operation"):
        loss.backward()
    with torch.no_grad():
        fc1.copy_(orig)

    # explicit invalidate + forward: a new generation of the arena
    loss = _train_forward(model, x)
    model._shadows.invalidate()
    with torch.no_grad():
        model(pixel_values=x)
    with pytest.raises(RuntimeError, match="parameters changed between this forward and its backward"):
        loss.backward()

    # and the model still trains afterwards
    model.zero_grad(set_to_none=True)
    _train_forward(model, x).backward()
    assert torch.equal(fc1.grad, want)


@pytest.mark.parametrize("transpose_cached", [True, False])
@pytest.mark.parametrize("N", [16, 9])
def test_decoder_linear_backward_after_a_weight_write_uses_its_forwards_weight(pkg, hiplib, transpose_cached, N):
    """``ctx.weight`` is an attribute, so autograd's saved-tensor check does not see a write of the weight between a
    linear's forward and its backward.  dX must still be dY · W_old: bit for bit the dX of a twin whose backward ran before
    the write.  Both orders: the transpose of W_old already cached at the write, and not yet."""
    ops = pkg.head_ops
    torch.manual_seed(N)
    lin = torch.nn.Linear(24, N).cuda()
    twin = copy.deepcopy(lin)
    x = torch.randn(64, 24, device="cuda").bfloat16()
    dy = torch.randn(64, N, device="cuda").bfloat16()

    def forward(m):
        xi = x.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = ops.linear_tokens(xi, m.weight, m.bias)
        assert len(_hip_linear_nodes(y.grad_fn)) == 1, "linear_tokens fell back to F.linear"
        return xi, y

    if transpose_cached:                     # an earlier forward + backward leaves Wᵀ in the cache
        xi, y = forward(lin)
        torch.autograd.grad(y, xi, dy)
        assert ops._weights._entries[lin.weight][2] is not None
    else:
        assert lin.weight not in ops._weights._entries
    xt, yt = forward(twin)
    want_dx, want_dw = torch.autograd.grad(yt, [xt, twin.weight], dy)

    xi, y = forward(lin)
    assert torch.equal(y, yt)
    if not transpose_cached:
        assert ops._weights._entries[lin.weight][2] is None
    with torch.no_grad():
        lin.weight.mul_(-2.0).add_(0.3)
    got_dx, got_dw = torch.autograd.grad(y, [xi, lin.weight], dy)
    assert torch.equal(got_dx, want_dx), "dX was computed with the weight written after the forward"
    assert torch.equal(got_dw, want_dw)
    # sensitivity: with the new weight dX is something else, and the next forward uses the new weight
    xn, yn = forward(lin)
    new_dx, = torch.autograd.grad(yn, xn, dy)
    assert not torch.equal(new_dx, want_dx) and not torch.equal(yn, y)
    fresh = copy.deepcopy(lin)
    xf, yf = forward(fresh)
    assert torch.equal(yn, yf) and torch.equal(new_dx, torch.autograd.grad(yf, xf, dy)[0])


def test_invalidate_weights_after_a_write_through_data(pkg, hiplib):
    """The untracked route: ``p.data.mul_`` moves no key, the decoder keeps its cast; the escape hatch
    ``head_ops.invalidate_weights(module)`` makes the next pass equal to the fresh twin's, as ``WeightShadows.invalidate``
    does for the encoder."""
    rig = Rig(pkg)
    keys = [(p.data_ptr(), p._version) for p in rig.both.parameters()]
    for p in rig.both.parameters():
        p.data.mul_(1.1)
    assert keys == [(p.data_ptr(), p._version) for p in rig.both.parameters()]
    stale = rig.run(rig.both)
    bad = differing(stale, rig.run(fresh_twin(rig.both)))
    assert any(k.startswith("infer.") for k in bad) and any(k.startswith("dec.") for k in bad), \
        "a write through p.data is documented as invisible to the keys"
    assert pkg.head_ops.invalidate_weights(rig.both["dec"]) == DEC_HIP_LINEARS
    rig.both["enc"]._shadows.invalidate()
    rig.verify("after the two explicit invalidations")
