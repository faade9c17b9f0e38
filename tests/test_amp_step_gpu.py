"""GPU: FusedAdamW under torch.amp.GradScaler (sgl_op_grad_norm_amp + sgl_op_adamw_amp, csrc/optimizer.hip): the loss
scale and the scaler's found-inf flag are read on the device, the true norm is clipped, an overflowing step stores
nothing and is counted on the device, and `scaler.step(opt)` makes no host synchronisation.

The tensor table of the kernel tests: the `hostile` encoder (tiled matrices with weight shadows and their transposes, fp32
bias copies) plus raw tensors of 1, 3, 4095, 4096, 4097 and 2*4096 + 5 elements and one 4 bytes off 16-byte alignment, cut
with their exp_avg / exp_avg_sq from an arena of sentinel words (guard bands), an EMA over everything, two parameter
groups with their own lr and weight decay, and a 1/world factor of 0.5."""
import math

import numpy as np
import pytest
import torch

import kernel_ref as kr
from test_kernel_edges_aux_gpu import Arena

pytestmark = pytest.mark.gpu
DEV = "cuda"
B1, B2, EPS = 0.9, 0.999, 1e-8
EXTRAS = [(1, False), (3, False), (4095, False), (4096, False), (4097, False), (2 * 4096 + 5, False), (4097, True)]
GROUPS = ((1e-3, 0.05), (3e-3, 0.01))          # (lr, weight decay) of the encoder's group and of the raw tensors'
MAX_NORM, WORLD, EMA_DECAY = 0.7, 0.5, 0.9


def bits(t):
    return t.detach().contiguous().view(-1).view(torch.uint8)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


class World:
    """The table above with a FusedAdamW on it; everything seeded, so two Worlds start bit-identical."""

    def __init__(self, pkg, mode="bf16", max_norm=MAX_NORM, world=WORLD):
        cfg = pkg.get_config("hostile")
        self.enc = pkg.SiglipVisionModelHIP(cfg, compute_dtype=mode)
        self.enc.load_state_dict(pkg.weights.seeded_state_dict(cfg, seed=3))
        self.enc.cuda()
        self.x = pkg.weights.seeded_pixels(2, cfg.image_size, cfg.image_size, seed=4).cuda()
        with torch.no_grad():
            self.enc(pixel_values=self.x)          # allocates the shadow arena the optimizer binds to
            # the arena has a few bytes between allocations that nothing ever writes: give them a known value, so that two
            # Worlds' arenas can be compared whole
            self.enc._shadows.arena.zero_()
            self.enc._shadows.invalidate()
            self.enc(pixel_values=self.x)
        g = torch.Generator().manual_seed(17)
        self.arena = Arena(sum(3 * (n + 40) for n, _ in EXTRAS) + 64)
        extras, seeded = [], []
        for n, off in EXTRAS:
            p, m, v = (self.arena.take(n, off) for _ in range(3))
            p.copy_(torch.randn(n, generator=g))
            m.zero_()
            v.zero_()
            extras.append(torch.nn.Parameter(p))
            seeded.append((m, v))
        self.holder = torch.nn.Module()
        self.holder.enc = self.enc
        self.holder.extras = torch.nn.ParameterList(extras)
        self.ema = pkg.ExponentialMovingAverage(self.holder, decay=EMA_DECAY)
        self.ema._flat.zero_()                     # the padding between the averages, as for the shadow arena
        for n, p in self.holder.named_parameters():
            self.ema.shadow[n].copy_(p.detach())
        enc_params = list(self.enc.parameters())
        self.params = enc_params + extras
        self.group_of = [0] * len(enc_params) + [1] * len(extras)
        self.opt = pkg.FusedAdamW([dict(params=enc_params, lr=GROUPS[0][0], weight_decay=GROUPS[0][1]),
                                   dict(params=extras, lr=GROUPS[1][0], weight_decay=GROUPS[1][1])],
                                  betas=(B1, B2), eps=EPS, max_grad_norm=max_norm, grad_scale=world)
        self.opt.attach_encoder(self.enc).attach_ema(self.ema)
        for p, (m, v) in zip(extras, seeded):      # exp_avg / exp_avg_sq between guard bands too
            self.opt.state[p] = dict(step=torch.tensor(0.0), exp_avg=m, exp_avg_sq=v)

    def grads(self, k, spikes):
        """True gradients of step k on the host.  `spikes`: the first element of every tensor is ~1e8, so that times 2^40 it
        is finite in fp32 and its square is not."""
        g = torch.Generator().manual_seed(100 + k)
        out = []
        for i, p in enumerate(self.params):
            t = torch.randn(p.shape, generator=g) * 0.01
            if spikes:
                t.view(-1)[0] = (1.0 + 0.1 * (i % 7)) * 1e8 * (-1.0 if i % 2 else 1.0)
            out.append(t)
        return out

    def set_grads(self, host, scale=1.0):
        for p, t in zip(self.params, host):
            p.grad = (t * scale).to(DEV)

    def amp_step(self, scale, found=0.0):
        """What GradScaler.step does with a `_step_supports_amp_scaling` optimizer."""
        self.opt.grad_scale = None if scale is None else torch.tensor(float(scale), device=DEV)
        self.opt.found_inf = torch.tensor(float(found), device=DEV)
        self.opt.step()
        del self.opt.grad_scale
        del self.opt.found_inf

    def moments(self, p):
        st = self.opt.state[p]
        return st["exp_avg"], st["exp_avg_sq"]

    def snapshot(self):
        s = {"arena": self.arena.buf.clone(), "shadows": self.enc._shadows.arena.clone(), "ema": self.ema._flat.clone()}
        for i, p in enumerate(self.enc.parameters()):
            s[f"p{i}"] = p.detach().clone()
            if p in self.opt.state and len(self.opt.state[p]):
                s[f"m{i}"], s[f"v{i}"] = (t.clone() for t in self.moments(p))
        return s

    def skipped(self):
        return int(self.opt._amp_state.view(torch.int32)[1].item())

    def device_constants(self):
        return self.opt._amp_state[2].item(), self.opt._amp_state[3].item()


def host_constants(b1, b2, t):
    """launch_adamw's (csrc/optimizer.hip): double arithmetic, rounded to float once."""
    return (float(np.float32(1.0 / (1.0 - b1 ** t))), float(np.float32(1.0 / math.sqrt(1.0 - b2 ** t))))


def ulps_apart(a, b):
    ia, ib = (int(np.float32(x).view(np.int32)) for x in (a, b))
    return abs(ia - ib)


def assert_step_matches_float64(w, before, host_g, coef, step, what):
    """Every p, exp_avg, exp_avg_sq element against kernel_ref.adamw_ref (the bounds sgl_op_adamw_ex is held to), and the
    EMA against its formula on the new parameter."""
    worst = 0.0
    ema_by_param = {id(p): w.ema.shadow[n] for n, p in w.holder.named_parameters()}
    for i, (p, g) in enumerate(zip(w.params, host_g)):
        lr, wd = GROUPS[w.group_of[i]]
        p0, m0, v0, e0 = before[i]
        refs = kr.adamw_ref(p0, g, m0, v0, lr, wd, B1, B2, EPS, step, coef)
        m1, v1 = w.moments(p)
        for name, got, (ref, bound) in zip("pmv", (p, m1, v1), refs):
            worst = max(worst, kr.assert_within(got.detach().cpu(), ref, bound, f"{what} tensor {i} {name}"))
        want = e0.double() * EMA_DECAY + p.detach().cpu().double() * (1.0 - EMA_DECAY)
        torch.testing.assert_close(ema_by_param[id(p)].cpu().double(), want, rtol=3e-7, atol=1e-9)
    return worst


def host_state(w):
    ema_by_param = {id(p): w.ema.shadow[n] for n, p in w.holder.named_parameters()}
    out = []
    for p in w.params:
        st = w.opt.state.get(p, {})
        m, v = (st["exp_avg"].cpu(), st["exp_avg_sq"].cpu()) if len(st) else (torch.zeros(p.shape), torch.zeros(p.shape))
        out.append((p.detach().cpu().clone(), m.clone(), v.clone(), ema_by_param[id(p)].cpu().clone()))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# scale invariance, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
def test_scale_invariance_bitwise(pkg, hiplib):
    """Scale 1 with g, 2^16 with g*2^16, 2^40 with g*2^40: the same bits in p, exp_avg, exp_avg_sq, shadows, EMA and the
    norm, over three steps.  g*2^40 is finite and (g*2^40)^2 is not: squaring before multiplying would skip these steps."""
    runs = {}
    for scale in (1.0, 2.0 ** 16, 2.0 ** 40):
        w = World(pkg)
        norms = []
        for k in range(3):
            g = w.grads(k, spikes=True)
            if scale == 2.0 ** 40:
                big = [t * scale for t in g]
                assert all(bool(torch.isfinite(t).all()) for t in big)
                assert all(bool(torch.isinf(t.square()).any()) for t in big)
            w.set_grads(g, scale)
            w.amp_step(scale)
            norms.append(w.opt.last_grad_norm.clone())
        assert w.skipped() == 0 and w.arena.guards_intact()
        assert all(bool(torch.isfinite(n)) for n in norms)
        runs[scale] = (w.snapshot(), norms)
    base, base_norms = runs[1.0]
    moved = World(pkg).snapshot()
    assert not same_bits(moved["shadows"], base["shadows"]) and not same_bits(moved["ema"], base["ema"])
    for scale in (2.0 ** 16, 2.0 ** 40):
        snap, norms = runs[scale]
        assert sorted(snap) == sorted(base)
        for k in base:
            assert same_bits(snap[k], base[k]), f"scale {scale}: {k} differs from scale 1"
        for a, b in zip(norms, base_norms):
            assert same_bits(a, b), f"scale {scale}: norm {a.item()} vs {b.item()}"


# ---------------------------------------------------------------------------------------------------------------------
# against float64, and against the unscaled entry points
# ---------------------------------------------------------------------------------------------------------------------
def test_amp_step_against_float64_and_the_unscaled_path(pkg, hiplib):
    scale = 2.0 ** 16
    w, plain = World(pkg), World(pkg)
    differing = total = 0
    for k in range(2):
        g = w.grads(k, spikes=False)
        before = host_state(w)
        w.set_grads(g, scale)
        w.amp_step(scale)
        nc = w.opt._bufs["norm"].cpu()
        # the norm: fp32 sums of <= 4096 squares (16 per thread in sequence, then the 8-level block tree), partials and
        # square root in double, one fp32 rounding and one product with 1/world: 16 + 8 + 2 roundings
        true_norm = WORLD * math.sqrt(sum(float(t.double().square().sum()) for t in g))
        assert abs(nc[0].item() - true_norm) <= 26 * 2.0 ** -24 * true_norm
        coef = nc[1].item() * scale                              # exact: the scale is a power of two
        want_coef = min(1.0, MAX_NORM / (nc[0].item() + 1e-6)) * WORLD
        assert abs(coef - want_coef) <= 4 * 2.0 ** -24 * want_coef
        worst = assert_step_matches_float64(w, before, g, coef, k + 1, f"amp step {k + 1}")
        print(f"[amp vs float64] step {k + 1}: worst err/bound {worst:.3f}, norm {nc[0].item():.6e}")
        dev_c, host_c = w.device_constants(), host_constants(B1, B2, k + 1)
        # the same step through sgl_op_grad_norm_scaled + sgl_op_adamw_ex on the true gradients
        plain.set_grads(g)
        plain.opt.step()
        a, b = w.snapshot(), plain.snapshot()
        per_key = {key: int((bits(a[key]).view(-1, a[key].element_size()) !=
                             bits(b[key]).view(-1, a[key].element_size())).any(1).sum()) for key in a}
        per_key = {key: n for key, n in per_key.items() if n}
        diff = sum(per_key.values())
        differing += diff
        total += sum(v.numel() for v in a.values())
        print(f"[amp vs unscaled path] step {k + 1}: {diff} elements differ bitwise {per_key}; device constants "
              f"{dev_c}, host {host_c}")
        if dev_c == host_c:      # the one legitimate source of a difference is a device pow one ulp from the host's
            assert diff == 0
        assert same_bits(w.opt._bufs["norm"][0], plain.opt._bufs["norm"][0])
    print(f"[amp vs unscaled path] {differing} of {total} elements differ bitwise over two steps")
    assert w.arena.guards_intact()


@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.9, 0.95)])
def test_device_bias_corrections_within_one_ulp_of_the_host(pkg, hiplib, betas):
    """state->inv_bc1 / inv_sqrt_bc2 at steps 1..64, 1000, 2000 and 100 000, with and without skipped steps."""
    L = pkg.lib
    steps = list(range(1, 65)) + [1000, 2000, 100000]
    cases = [(t, 0) for t in steps] + [(t + 3, 3) for t in steps]          # (step argument, skipped so far)
    states = torch.zeros(len(cases), 8, device=DEV)
    states.view(torch.int32)[:, 1] = torch.tensor([s for _, s in cases], dtype=torch.int32, device=DEV)
    scratch = torch.zeros(4, device=DEV)
    table = (L.SglAdamwTensor * 1)()
    table[0].p = table[0].m = table[0].v = scratch.data_ptr()
    table[0].g, table[0].n = None, 1                       # no gradient: the update kernel stores nothing
    dev_table = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(DEV)
    dev_aux = torch.zeros(C_SIZEOF_AUX(L), dtype=torch.uint8, device=DEV)
    bmap = torch.zeros(2, dtype=torch.int32, device=DEV)
    for row, (step, _) in enumerate(cases):
        L.call("sgl_op_adamw_amp", torch.device(DEV, 0), dev_table.data_ptr(), dev_aux.data_ptr(), bmap.data_ptr(), 1,
               betas[0], betas[1], EPS, step, None, None, 0, 0.0, states[row].data_ptr())
    got = states.cpu()
    assert bool((scratch == 0).all())
    worst = 0
    for row, (step, skipped) in enumerate(cases):
        want = host_constants(betas[0], betas[1], step - skipped)
        for j in (0, 1):
            d = ulps_apart(got[row, 2 + j].item(), want[j])
            worst = max(worst, d)
            assert d <= 1, f"betas {betas} step {step} skipped {skipped}: {got[row, 2 + j].item()!r} vs {want[j]!r}"
        assert got[row].view(torch.int32)[1].item() == skipped and got[row, 0].item() == 0.0
    print(f"[device bias corrections] betas {betas}: worst distance {worst} ulp over {len(cases)} launches")


def C_SIZEOF_AUX(L):
    import ctypes
    return ctypes.sizeof(L.SglAdamwAux)


# ---------------------------------------------------------------------------------------------------------------------
# skipped steps
# ---------------------------------------------------------------------------------------------------------------------
def test_skipped_steps_store_nothing_and_do_not_advance_the_step(pkg, hiplib):
    """inf, then NaN, at the first element of the table, the last one and the tail element of a 4097-element tensor, and
    finite gradients with the scaler's own flag set: nothing is stored anywhere (guard bands included), the device counts
    one skip each time, and the next finite step is step 2 of an AdamW that never saw the skipped ones."""
    scale = 2.0 ** 16
    w = World(pkg)
    g0 = w.grads(0, spikes=False)
    w.set_grads(g0, scale)
    w.amp_step(scale)
    assert w.skipped() == 0
    snap = w.snapshot()
    tail_tensor = len(w.params) - len(EXTRAS) + 4              # the aligned 4097-element tensor
    spots = {"first": (0, 0), "last": (len(w.params) - 1, -1), "tail": (tail_tensor, 4096)}
    count = 0
    for bad in (float("inf"), float("nan")):
        for where, (ti, ei) in spots.items():
            g = w.grads(50 + count, spikes=False)
            g[ti].view(-1)[ei] = bad
            w.set_grads(g, scale)
            w.amp_step(scale)
            count += 1
            now = w.snapshot()
            for key in snap:
                assert same_bits(now[key], snap[key]), f"{bad} at the {where} element: {key} was written"
            assert w.skipped() == count, f"{bad} at the {where} element"
            assert not bool(torch.isfinite(w.opt.last_grad_norm)), "the true norm of an overflowing step is inf / NaN"
    w.set_grads(w.grads(60, spikes=False), scale)
    w.amp_step(scale, found=1.0)                                # the scaler found it, the gradients here are finite
    count += 1
    now = w.snapshot()
    for key in snap:
        assert same_bits(now[key], snap[key]), f"found_inf = 1: {key} was written"
    assert w.skipped() == count == 7 and w.arena.guards_intact()
    # the next finite step: call 9 of the optimizer, step 2 of the mathematics
    g1 = w.grads(1, spikes=False)
    before = host_state(w)
    w.set_grads(g1, scale)
    w.amp_step(scale)
    assert w.skipped() == count
    coef = w.opt._bufs["norm"][1].item() * scale
    worst = assert_step_matches_float64(w, before, g1, coef, 2, "first step after the skipped ones")
    for j, (got, want) in enumerate(zip(w.device_constants(), host_constants(B1, B2, 2))):
        assert ulps_apart(got, want) <= 1, (j, got, want)
    print(f"[skip] step after 7 skipped ones: worst err/bound {worst:.3f} with the bias corrections of step 2")
    assert w.arena.guards_intact()
    # checkpoints: the count is folded into every tensor's step, as torch.optim.AdamW would have counted
    sd = w.opt.state_dict()
    assert len(sd["state"]) == len(w.params)
    assert all(float(st["step"]) == 2.0 for st in sd["state"].values())
    assert w.skipped() == 0
    w.opt.load_state_dict(sd)
    assert w.skipped() == 0


def test_a_tensor_that_joins_later_does_not_inherit_skips(pkg, hiplib):
    """p2 gets its first gradient after a skipped step: against torch.optim.AdamW on the CPU, which never saw that step."""
    torch.manual_seed(3)
    init = [torch.randn(300), torch.randn(5000)]
    ref_p = [torch.nn.Parameter(t.clone()) for t in init]
    dev_p = [torch.nn.Parameter(t.clone().cuda()) for t in init]
    ref = torch.optim.AdamW(ref_p, lr=1e-2, weight_decay=0.01)
    opt = pkg.FusedAdamW(dev_p, lr=1e-2, weight_decay=0.01)
    scale = 1024.0
    plan = [((True, False), False), ((True, False), True), ((True, True), False), ((True, True), False)]
    for members, overflow in plan:
        for has, r, d in zip(members, ref_p, dev_p):
            g = torch.randn(r.shape) if has else None
            r.grad = None if (g is None or overflow) else g.clone()
            d.grad = None if g is None else (g * scale).cuda()
            if overflow and g is not None:
                d.grad[-1] = float("inf")
        if not overflow:
            ref.step()
        opt.grad_scale, opt.found_inf = torch.tensor(scale, device=DEV), torch.zeros((), device=DEV)
        opt.step()
        del opt.grad_scale, opt.found_inf
    for r, d in zip(ref_p, dev_p):
        torch.testing.assert_close(d.detach().cpu(), r.detach(), rtol=2e-6, atol=2e-7)
    steps = [float(st["step"]) for st in opt.state_dict()["state"].values()]
    assert steps == [3.0, 2.0] == [float(ref.state[p]["step"]) for p in ref_p]


# ---------------------------------------------------------------------------------------------------------------------
# stale shadows
# ---------------------------------------------------------------------------------------------------------------------
def test_a_skipped_step_does_not_adopt_stale_shadows(pkg, hiplib):
    """A weight changed behind the shadows' back, then a skipped AMP step: the next forward must re-cast that unit (its
    output is that of a freshly built encoder with the same weights)."""
    w = World(pkg, max_norm=None, world=1.0)
    with torch.no_grad():
        w.enc.encoder.layers[0].mlp.fc1.weight.mul_(1.01)
    assert w.enc._shadows.units_in_sync()[0] is False
    g = w.grads(0, spikes=False)
    g[3].view(-1)[0] = float("inf")
    w.set_grads(g, 2.0 ** 16)
    w.amp_step(2.0 ** 16)
    assert w.skipped() == 1
    with torch.no_grad():
        got = w.enc(pixel_values=w.x).pooler_output.clone()
    fresh = pkg.SiglipVisionModelHIP(w.enc.config, compute_dtype="bf16")
    fresh.load_state_dict(w.enc.state_dict())
    fresh.cuda()
    with torch.no_grad():
        want = fresh(pixel_values=w.x).pooler_output
    assert torch.equal(got, want), (got - want).abs().max()


# ---------------------------------------------------------------------------------------------------------------------
# end to end on `hostile`: data, bounds and oracle of tests/test_fp16_gpu.py::test_fp16_autocast_gradscaler_training
# ---------------------------------------------------------------------------------------------------------------------
LR, WD, CLIP, SEED = 2e-3, 0.05, 1.0, 11
_REF = {}


def _frozen(name, freeze_below):
    return freeze_below > 0 and (name.startswith("embeddings.") or
                                 any(name.startswith(f"encoder.layers.{i}.") for i in range(freeze_below)))


def _data(pkg):
    cfg = pkg.get_config("hostile")
    torch.manual_seed(0)
    head0 = torch.nn.Linear(cfg.hidden_size, 1)
    x = pkg.weights.seeded_pixels(4, cfg.image_size, cfg.image_size, seed=5)
    y = torch.tensor([[0.0], [1.0], [1.0], [0.0]])
    return cfg, head0, x, y


def _reference(pkg, oracle, freeze_below):
    """Four steps of the fp32 CPU oracle with torch.optim.AdamW and torch's clip, computed once per freezing: the losses
    and the parameters after steps 3 and 4."""
    if freeze_below not in _REF:
        cfg, head0, x, y = _data(pkg)
        sd0 = pkg.weights.seeded_state_dict(cfg, seed=SEED)
        ref = {k: v.clone().requires_grad_(not _frozen(k, freeze_below)) for k, v in sd0.items()}
        rhead = torch.nn.Linear(cfg.hidden_size, 1)
        rhead.load_state_dict(head0.state_dict())
        rparams = [v for v in ref.values() if v.requires_grad] + list(rhead.parameters())
        ropt = torch.optim.AdamW(rparams, lr=LR, weight_decay=WD)
        losses, after = [], {}
        for k in range(4):
            out = oracle.vision_forward(x, ref, cfg, False, False)
            loss = torch.nn.functional.binary_cross_entropy_with_logits(rhead(out["pooler_output"]), y)
            ropt.zero_grad()
            loss.backward()
            torch.nn.utils.clip_grad_norm_(rparams, CLIP)
            ropt.step()
            losses.append(loss.item())
            if k >= 2:
                after[k + 1] = {n: v.detach().clone() for n, v in ref.items()}
        _REF[freeze_below] = (sd0, losses, after, {k: v.requires_grad for k, v in ref.items()})
    return _REF[freeze_below]


def _worst_moved_relative(cfg, model, sd0, after, trainable):
    got = {k[len("vision_model."):]: v for k, v in model.visual.state_dict().items()}
    worst, who = 0.0, None
    for k, v in after.items():
        if not trainable[k]:
            assert torch.equal(got[k].cpu(), sd0[k]), k
            continue
        if k.endswith("k_proj.bias"):
            continue   # exactly-zero gradient in real arithmetic: Adam moves it by +-lr on noise
        diff, moved = got[k].cpu() - v, v - sd0[k]
        if k == "head.attention.in_proj_bias":
            diff[cfg.hidden_size:2 * cfg.hidden_size] = 0
        r = diff.norm().item() / (moved.norm().item() + 1e-12)
        if r > worst:
            worst, who = r, k
    return worst, who


E2E = [("fp16", fb, form) for fb in (0, 1) for form in ("five_lines", "stock_short", "amd_short")] + \
      [("bf16", 0, "amd_short")]


@pytest.mark.parametrize("mode,freeze_below,form", E2E, ids=[f"{m}-freeze{f}-{s}" for m, f, s in E2E])
def test_gradscaler_training_end_to_end(pkg, oracle, hiplib, mode, freeze_below, form):
    """Three steps against the fp32 CPU oracle (bounds of test_fp16_autocast_gradscaler_training: loss 1.5e-2 relative,
    moved-relative 0.17), an overflowing step at init_scale 2^40 (the scale halves, every weight keeps its bits, the next
    forward is bit-equal), one more step that still matches the oracle.  In bf16 nothing overflows at 2^40 (fp32's
    exponent range), so there that step must be taken, not skipped, and is the fourth step of the oracle.  The short forms run every `scaler.step(opt)`
    under torch.cuda.set_sync_debug_mode("error"); the parent's route stops there at `found_inf.item()`."""
    cfg, head0, x, y = _data(pkg)
    sd0, ref_losses, after, trainable = _reference(pkg, oracle, freeze_below)
    model, _, _ = pkg.create_model_and_transforms("hostile", device="cuda", compute_dtype=mode, seed=SEED)
    for n, p in model.visual.named_parameters():
        p.requires_grad = not _frozen(n, freeze_below)
    head = torch.nn.Linear(cfg.hidden_size, 1).cuda()
    head.load_state_dict(head0.state_dict())
    params = [p for p in model.parameters() if p.requires_grad] + list(head.parameters())
    short = form != "five_lines"
    opt = pkg.FusedAdamW(params, lr=LR, weight_decay=WD, max_grad_norm=CLIP if short else None)
    opt.attach_encoder(model.visual)
    Scaler = pkg.GradScaler if form == "amd_short" else torch.amp.GradScaler
    scaler = Scaler("cuda")
    xd, yd = x.cuda(), y.cuda()
    ac_dtype = torch.float16 if mode == "fp16" else torch.bfloat16

    def step(scaler):
        with torch.amp.autocast("cuda", dtype=ac_dtype):
            logits = head(model.encode_image(xd))
            loss = torch.nn.functional.binary_cross_entropy_with_logits(logits.float(), yd)
        opt.zero_grad(set_to_none=True)
        scaler.scale(loss).backward()
        if not short:
            scaler.unscale_(opt)
            torch.nn.utils.clip_grad_norm_(params, CLIP)
        before = torch.cuda.get_sync_debug_mode()
        try:
            if short:
                torch.cuda.set_sync_debug_mode("error")
            scaler.step(opt)
        finally:
            torch.cuda.set_sync_debug_mode(before)
        scaler.update()
        return loss.item()

    losses = [step(scaler) for _ in range(3)]
    rel = [abs(a - b) / abs(b) for a, b in zip(losses, ref_losses)]
    worst, who = _worst_moved_relative(cfg, model, sd0, after[3], trainable)
    print(f"[amp e2e {mode} freeze={freeze_below} {form}] loss rel errs {[f'{e:.2e}' for e in rel]}, worst "
          f"moved-relative {worst:.3e} ({who}), scale {scaler.get_scale():.0f}")
    assert max(rel) <= 1.5e-2, (losses, ref_losses)
    assert worst <= 0.17, (worst, who)

    over = Scaler("cuda", init_scale=2.0 ** 40)
    if mode == "bf16":
        # bf16 has fp32's exponent range: gradients scaled by 2^40 are finite, only their squares are not.  This is the
        # step the multiply-before-square of the norm pass exists for: it must NOT be skipped, and it is step 4.
        loss4 = step(over)
        assert over.get_scale() == 2.0 ** 40, "a finite step was skipped"
        rel4 = abs(loss4 - ref_losses[3]) / abs(ref_losses[3])
        worst4, who4 = _worst_moved_relative(cfg, model, sd0, after[4], trainable)
        print(f"[amp e2e bf16 {form}] step at scale 2^40: loss rel err {rel4:.2e}, worst moved-relative {worst4:.3e} "
              f"({who4}), true norm {opt.last_grad_norm.item():.3e}")
        # The parameters are what this step wrote: the bound of the three steps above.  The loss was computed BEFORE the
        # step, by a bf16 forward at a loss of about 1e-3: the fp16 bound scaled by the ratio of the unit roundoffs
        # (2^-8 / 2^-11 = 8), since the forward's error is linear in it to first order.  Measured: 2.7e-2 (fp16: 7.3e-3).
        assert worst4 <= 0.17, (worst4, who4)
        assert rel4 <= 8 * 1.5e-2, (loss4, ref_losses[3])
        assert all(float(st["step"]) == 4.0 for st in opt.state_dict()["state"].values())
        return
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    hbefore = {k: v.detach().clone() for k, v in head.state_dict().items()}
    with torch.no_grad():
        f0 = model.encode_image(xd).clone()
    step(over)
    assert over.get_scale() == 2.0 ** 39, "the scaler must find the overflow and back off"
    for k, v in model.state_dict().items():
        assert torch.equal(v, before[k]), f"{k} changed in a skipped step"
    for k, v in head.state_dict().items():
        assert torch.equal(v, hbefore[k]), k
    with torch.no_grad():
        f1 = model.encode_image(xd)
    assert torch.equal(f0, f1), "forward after the skipped step differs"

    loss4 = step(scaler)
    rel4 = abs(loss4 - ref_losses[3]) / abs(ref_losses[3])
    worst4, who4 = _worst_moved_relative(cfg, model, sd0, after[4], trainable)
    print(f"[amp e2e {mode} freeze={freeze_below} {form}] step after the skipped one: loss rel err {rel4:.2e}, worst "
          f"moved-relative {worst4:.3e} ({who4})")
    assert rel4 <= 1.5e-2, (loss4, ref_losses[3])
    assert worst4 <= 0.17, (worst4, who4)
    assert all(float(st["step"]) == 4.0 for st in opt.state_dict()["state"].values())
