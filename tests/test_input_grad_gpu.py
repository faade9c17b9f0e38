"""GPU: d loss / d pixel_values through col2im, the patch GEMM's dX, sgl_backward_embed_px and the autograd plumbing.

Bars (the ones this project already holds gradients to, tests/test_encoder_gpu.py / test_parity_bf16_gpu.py):
  fp32    max|err| <= 1e-7 + 6e-5 * max|ref|        bf16x3  six times the relative part
  bf16    rel-L2 <= 2x and max|err| <= 3x what the real HF model makes under CPU bf16 autocast on the same elements
  fp16    the same against HF under fp16 autocast
The reference is tests/golden/pixgrad (HF SiglipVisionModel in fp32), or the CPU oracle where no fixture has the case.
Each test prints what it measured before it asserts.
"""
import copy
import ctypes as C

import pytest
import torch

import abi_harness as ah
import golden_util as gu
import pixgrad_util as pg

pytestmark = pytest.mark.gpu

MODES = ["fp32", "bf16x3", "bf16", "fp16"]
AC = {"bf16": "bf16ac.", "fp16": "fp16ac."}


def build(pkg, cfg_name, seed, mode, recompute=False):
    cfg = pkg.get_config(cfg_name)
    model = pkg.SiglipVisionModelHIP(cfg, compute_dtype=mode, recompute=recompute)
    model.load_state_dict(pkg.weights.seeded_state_dict(cfg, seed=seed))
    return model.to("cuda")


def case_run(pkg, rec, mode, want_px=True, frozen=False, recompute=False, channels_last=False):
    """Forward + probe-loss backward of a fixture's case.  Returns (out, d_pixels or None, {name: grad}, model)."""
    m = gu.meta(rec)
    model = build(pkg, m["config"], m["seed"], mode, recompute)
    if frozen:
        model.requires_grad_(False)
    x = pkg.weights.seeded_pixels(m["batch"], m["res_h"], m["res_w"], seed=m["seed"] + 1000).cuda()
    if channels_last:
        x = x.contiguous(memory_format=torch.channels_last)
    x.requires_grad_(want_px)
    out = model(pixel_values=x, output_hidden_states=True, interpolate_pos_encoding=m["interp"])
    pg.probe_loss(out, m["taps"]).backward()
    torch.cuda.synchronize()
    grads = {n: p.grad for n, p in model.named_parameters() if p.grad is not None}
    return out, x.grad, grads, model


def strict_bar(ref_absmax, mode):
    return 1e-7 + 6e-5 * (6.0 if mode == "bf16x3" else 1.0) * ref_absmax


def check_against_fixture(rec, mode, d_pixels, tag, maxerr_bar=True):
    """Bar 2 of the module docstring.  Returns the measured (ratio or error) for the print-out."""
    d = d_pixels.detach().float().cpu().contiguous()
    maxerr, l2 = gu.err_stats(rec, pg.PREFIX, d)
    scale = pg.ref_absmax(rec)
    if mode in ("fp32", "bf16x3"):
        bar = strict_bar(scale, mode)
        print(f"[{tag}/{mode}] d_pixels max|err| {maxerr:.3e} (bar {bar:.3e}, {maxerr / bar:.2f} of it), rel-L2 {l2:.3e}, "
              f"max|ref| {scale:.3e}")
        gu.compare(rec, pg.PREFIX, d, 1e-7, 6e-5 * (6.0 if mode == "bf16x3" else 1.0))
        return maxerr / bar
    hf_max, hf_l2 = float(rec[AC[mode] + pg.PREFIX + ".maxerr"]), float(rec[AC[mode] + pg.PREFIX + ".l2rel"])
    print(f"[{tag}/{mode}] d_pixels rel-L2 {l2:.3e} = {l2 / hf_l2:.2f}x HF-autocast ({hf_l2:.3e}; bar 2x), max|err| "
          f"{maxerr:.3e} = {maxerr / hf_max:.2f}x HF-autocast ({hf_max:.3e}; bar 3x)")
    assert l2 <= 2.0 * hf_l2, f"{tag}/{mode}: rel-L2 {l2:.3e} > 2 x {hf_l2:.3e}"
    if maxerr_bar:
        assert maxerr <= 3.0 * hf_max, f"{tag}/{mode}: max|err| {maxerr:.3e} > 3 x {hf_max:.3e}"
    return l2 / hf_l2


def border_is_zero(d_pixels, P):
    B, _, H, W = d_pixels.shape
    mask = pg.border_mask(B, H, W, P).to(d_pixels.device)
    return bool((d_pixels[mask] == 0).all())


# ---- 1. col2im alone ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels_last", [0, 1])
@pytest.mark.parametrize("P,Kp,H,W", [(14, 640, 42, 56), (14, 640, 59, 101), (14, 640, 45, 60), (14, 704, 384, 384),
                                      (16, 768, 32, 48), (16, 832, 37, 45), (16, 832, 40, 52), (16, 768, 512, 512)])
def test_col2im_inverts_im2col_bitwise(pkg, hiplib, P, Kp, H, W, channels_last):
    B = 2
    gh, gw = H // P, W // P
    K0 = 3 * P * P
    torch.manual_seed(P * 1000 + H + W)
    x = torch.randn(B, 3, H, W, device="cuda")
    xs = x.contiguous(memory_format=torch.channels_last) if channels_last else x    # storage the kernels see
    cols = torch.empty(B * gh * gw, Kp, device="cuda")
    s = ah.stream()
    assert hiplib.sgl_op_im2col(xs.data_ptr(), channels_last, cols.data_ptr(), 0, B, H, W, P, Kp, s) == ah.OK
    cols[:, K0:] = float("nan")                        # pad columns are never read
    out = ah.Arena(B * 3 * H * W * 4, 0xFF)            # payload and guards 0xFF (NaN): every pixel must be written
    assert hiplib.sgl_op_col2im(cols.data_ptr(), B, H, W, P, Kp, out.ptr, channels_last, s) == ah.OK
    torch.cuda.synchronize()
    assert out.guards_intact()
    got = out.f32(B, H, W, 3).permute(0, 3, 1, 2) if channels_last else out.f32(B, 3, H, W)
    covered = ~pg.border_mask(B, H, W, P).cuda()
    assert torch.equal(got[covered].view(torch.int32), x[covered].view(torch.int32))      # bit for bit
    assert bool((got[~covered].view(torch.int32) == 0).all())                              # +0.0 exactly
    assert hiplib.sgl_op_col2im(None, B, H, W, P, Kp, out.ptr, channels_last, s) == ah.ERR_NULL
    assert hiplib.sgl_op_col2im(cols.data_ptr(), B, H, W, P, K0 - 1, out.ptr, channels_last, s) == ah.ERR_UNSUPPORTED
    assert hiplib.sgl_op_col2im(cols.data_ptr(), B, H, W, P, Kp, out.ptr, 2, s) == ah.ERR_UNSUPPORTED


# ---- 2. golden parity --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pg.SMALL_CASES)
@pytest.mark.parametrize("mode", MODES)
def test_pixel_gradient_vs_hf_fixture(case, mode, pkg, hiplib):
    rec = pg.load(case)
    _, d, grads, model = case_run(pkg, rec, mode)
    assert d is not None and d.dtype == torch.float32 and bool(torch.isfinite(d).all())
    assert border_is_zero(d, model.config.patch_size)
    assert "embeddings.patch_embedding.weight" in grads            # the parameters got theirs as well
    check_against_fixture(rec, mode, d, case)


@pytest.mark.parametrize("mode", MODES)
def test_pixel_gradient_with_the_dx_gemm_on_the_256_tile(mode, pkg, oracle, hiplib):
    """so400m-1layer at 384 px, B = 3: 2187 tokens, so the dX product [2187 x 640 x 1152] takes the 256x256-tile kernel
    (M >= 2048, N >= 256), with a partial tile in both M and N; every fixture has fewer tokens.  Reference: the CPU oracle.
    16-bit bar: twice HF-autocast's rel-L2 on the so400m1_384 fixture (same model and resolution, B = 1)."""
    rec = pg.load("so400m1_384")
    m = gu.meta(rec)
    cfg = pkg.get_config(m["config"])
    sd = pkg.weights.seeded_state_dict(cfg, seed=m["seed"])
    x_cpu = pkg.weights.seeded_pixels(3, 384, 384, seed=2187)
    model = build(pkg, m["config"], m["seed"], mode).requires_grad_(False)
    x = x_cpu.cuda().requires_grad_(True)
    out = model(pixel_values=x, output_hidden_states=True, interpolate_pos_encoding=True)
    pg.probe_loss(out, m["taps"]).backward()
    xr = x_cpu.clone().requires_grad_(True)
    torch.set_num_threads(8)
    oracle.probe_loss(oracle.vision_forward(xr, sd, cfg, True, True), m["taps"]).backward()
    d, r = x.grad.cpu(), xr.grad
    err, l2 = (d - r).abs().max().item(), ((d - r).norm() / r.norm()).item()
    assert border_is_zero(x.grad, cfg.patch_size)
    if mode in ("fp32", "bf16x3"):
        bar = strict_bar(r.abs().max().item(), mode)
        print(f"[so400m1 B=3/{mode}] d_pixels vs oracle max|err| {err:.3e} (bar {bar:.3e}, {err / bar:.2f} of it), rel-L2 {l2:.3e}")
        assert err <= bar
    else:
        hf = float(rec[AC[mode] + pg.PREFIX + ".l2rel"])
        print(f"[so400m1 B=3/{mode}] d_pixels vs oracle rel-L2 {l2:.3e} = {l2 / hf:.2f}x HF-autocast at B=1 ({hf:.3e}; bar 2x)")
        assert l2 <= 2.0 * hf


# ---- 3. nothing else moves ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_asking_for_d_pixels_changes_no_output_and_no_parameter_gradient(mode, pkg, hiplib):
    rec = pg.load("hostile_59x101_interp")
    out_a, d_a, grads_a, _ = case_run(pkg, rec, mode, want_px=False)
    out_b, d_b, grads_b, _ = case_run(pkg, rec, mode, want_px=True)
    assert d_a is None and d_b is not None
    assert torch.equal(out_a.pooler_output, out_b.pooler_output)
    assert torch.equal(out_a.last_hidden_state, out_b.last_hidden_state)
    for a, b in zip(out_a.hidden_states, out_b.hidden_states):
        assert torch.equal(a, b)
    assert set(grads_a) == set(grads_b) and len(grads_a) > 40
    for n in grads_a:
        assert torch.equal(grads_a[n], grads_b[n]), n


# ---- 4. frozen encoder -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["hostile_59x101_interp", "tiny_32", "so400m1_224_interp"])
@pytest.mark.parametrize("mode", MODES)
def test_frozen_encoder_gives_the_same_bits(case, mode, pkg, hiplib):
    rec = pg.load(case)
    _, d_train, _, _ = case_run(pkg, rec, mode)
    _, d_frozen, grads, model = case_run(pkg, rec, mode, frozen=True)
    assert not grads and all(p.grad is None for p in model.parameters())
    assert bool(torch.isfinite(d_frozen).all())
    same = torch.equal(d_train, d_frozen)
    _, d_rc, grads_rc, _ = case_run(pkg, rec, mode, frozen=True, recompute=True)
    assert not grads_rc
    same_rc = torch.equal(d_frozen, d_rc)
    print(f"[{case}/{mode}] frozen == trainable: {same} (max diff {(d_train - d_frozen).abs().max().item():.3e}); "
          f"frozen recompute == frozen: {same_rc} (max diff {(d_rc - d_frozen).abs().max().item():.3e})")
    assert same, "d_pixels of the frozen encoder differs from the trainable run"
    assert same_rc, "d_pixels of the frozen encoder differs under recompute=True"


# ---- 5. frozen prefix --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_frozen_prefix_with_taps_below_it(mode, pkg, hiplib):
    """tiny (3 blocks): embeddings and blocks 0, 1 frozen, block 2 and the head train; the loss reads hidden_states[1] and
    [2] (SID-style taps at or below the first trainable block), which reach nothing but the pixels."""
    rec = pg.load(pg.PREFIX_CASE)
    m = gu.meta(rec)
    cfg = pkg.get_config(m["config"])
    k, taps, B, H, W = 2, m["taps"], m["batch"], m["res_h"], m["res_w"]
    assert taps == (1, 2) and all(t <= k for t in taps)
    sd = pkg.weights.seeded_state_dict(cfg, seed=m["seed"])
    x_cpu = pkg.weights.seeded_pixels(B, H, W, seed=m["seed"] + 1000)

    def run(want_px):
        model = pkg.SiglipVisionModelHIP(cfg, compute_dtype=mode)
        model.load_state_dict(sd)
        model = model.to("cuda")
        for p in model.vision_model.embeddings.parameters():
            p.requires_grad = False
        for i, layer in enumerate(model.vision_model.encoder.layers):
            for p in layer.parameters():
                p.requires_grad = i >= k
        x = x_cpu.cuda().requires_grad_(want_px)
        out = model(pixel_values=x, hidden_state_ids=[1, 2], interpolate_pos_encoding=True)
        hs = {1: out.hidden_states[0], 2: out.hidden_states[1]}
        shim = type("O", (), dict(pooler_output=out.pooler_output, last_hidden_state=out.last_hidden_state, hidden_states=hs))
        pg.probe_loss(shim, taps).backward()
        torch.cuda.synchronize()
        return x.grad, {n: p.grad for n, p in model.named_parameters() if p.grad is not None}

    d_none, g_plain = run(False)
    d, g_px = run(True)
    assert d_none is None and set(g_plain) == set(g_px) and g_plain
    assert not any(n.startswith(("embeddings.", "encoder.layers.0.", "encoder.layers.1.")) for n in g_px)
    for n in g_plain:
        assert torch.equal(g_plain[n], g_px[n]), n                  # the trainable blocks' gradients: bit-identical
    # bar 2 against HF's own input gradient for this shape, seed and taps (it does not depend on what is frozen)
    assert border_is_zero(d, cfg.patch_size)
    check_against_fixture(rec, mode, d, "frozen prefix")


# ---- 6. NCHW vs channels_last ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["hostile_59x101_interp", "tiny_32x48_interp"])
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_channels_last_input_gives_identical_values_in_its_own_format(case, mode, pkg, hiplib):
    rec = pg.load(case)
    m = gu.meta(rec)
    model = build(pkg, m["config"], m["seed"], mode)
    model.requires_grad_(False)
    x = pkg.weights.seeded_pixels(m["batch"], m["res_h"], m["res_w"], seed=m["seed"] + 1000).cuda()
    got = []
    for fmt in (torch.contiguous_format, torch.channels_last):
        xi = x.contiguous(memory_format=fmt).requires_grad_(True)
        out = model(pixel_values=xi, output_hidden_states=True, interpolate_pos_encoding=m["interp"])
        (g,) = torch.autograd.grad(pg.probe_loss(out, m["taps"]), xi)
        assert g.is_contiguous(memory_format=fmt) and g.shape == xi.shape
        got.append(g)
    assert torch.equal(got[0], got[1])


# ---- 7. raw ABI --------------------------------------------------------------------------------------------------
def _abi_input_gradient(pkg, hiplib, cfg_name, mode, recompute, B, H, W, fill, frozen, channels_last=0):
    lib = hiplib
    with ah.Session(pkg, lib, cfg_name, mode, recompute=recompute, seed=17) as ses:
        shadow = ses.new_shadow(fill)
        assert ses.prepare(shadow, full=True) == ah.OK
        run = ah.Run(ses, B, H, W, train=True, fill=fill, kind="slots")
        px = ses.pixels(B, H, W, seed=3)
        if channels_last:
            px = px.contiguous(memory_format=torch.channels_last)
        assert ses.forward(run, shadow, px, kind="slots", channels_last=channels_last) == ah.OK
        present = {n: False for n in pkg.weights.param_shapes(ses.cfg)} if frozen else None
        grads = ah.Grads(ses, present=present, fill=fill)
        L, D = ses.Lyr, ses.D
        up = ah.upstream(B, run.N, D, L, (0, L))
        d_last, d_pooled = up["last"].cuda().contiguous(), up["pooled"].cuda()
        taps = {l: t.cuda().contiguous() for l, t in up["taps"].items()}
        p = lambda t: None if t is None else t.data_ptr()
        tail = (run.saved.ptr, run.saved.nbytes, run.ws.ptr, run.ws.nbytes, ah.stream())
        wsg = (ses.ctx, C.byref(ses.w), shadow.ptr, C.byref(grads.struct))
        assert lib.sgl_backward_begin_p(*wsg, B, H, W, run.hidden_ptr(L), p(d_last), p(d_pooled), p(taps.get(L)),
                                        *tail) == ah.OK
        for l in range(L - 1, -1, -1):
            assert lib.sgl_backward_layer_p(*wsg, l, B, H, W, run.hidden_ptr(l), p(taps.get(l)), 1, *tail) == ah.OK
        n = C.c_size_t()
        assert lib.sgl_query_input_grad_bytes(ses.ctx, B, H, W, C.byref(n)) == ah.OK
        dpx = ah.Arena(B * 3 * H * W * 4, fill)                     # exact payloads between 64 KiB guards
        scratch = ah.Arena(n.value, fill)
        st = lib.sgl_backward_embed_px(ses.ctx, C.byref(ses.w), C.byref(grads.struct), B, H, W, 1, dpx.ptr, channels_last,
                                       scratch.ptr, scratch.nbytes, *tail)
        assert st == ah.OK
        torch.cuda.synchronize()
        ah.assert_guards(run.arenas() + grads.arenas() + [("d_pixels", dpx), ("px_scratch", scratch), ("shadow", shadow)],
                         f"{cfg_name}/{mode}/rc{recompute}/fill{fill:#x}")
        d = dpx.f32(B, H, W, 3).permute(0, 3, 1, 2) if channels_last else dpx.f32(B, 3, H, W)
        return d.clone(), grads.gpu()


@pytest.mark.parametrize("recompute", [0, 1])
@pytest.mark.parametrize("mode", ah.TRAIN_MODES)
def test_abi_embed_px_on_guarded_poisoned_arenas(pkg, hiplib, mode, recompute):
    B, H, W = 3, 101, 59
    res = {}
    for frozen in (True, False):
        for fill in (0x00, 0xFF):
            res[frozen, fill] = _abi_input_gradient(pkg, hiplib, "hostile", mode, recompute, B, H, W, fill, frozen)
    for frozen in (True, False):
        d0, g0 = res[frozen, 0x00]
        d1, g1 = res[frozen, 0xFF]
        assert bool(torch.isfinite(d0).all()) and torch.equal(d0, d1)          # nothing read that was not written
        assert d0.abs().max().item() > 0 and border_is_zero(d0, 14)
        assert set(g0) == set(g1) and (len(g0) == 0) == frozen
        for k in g0:
            assert bool(torch.isfinite(g0[k]).all()) and torch.equal(g0[k], g1[k]), k
    assert torch.equal(res[True, 0x00][0], res[False, 0x00][0])               # NULL destinations change no bit of d_pixels
    d_cl, _ = _abi_input_gradient(pkg, hiplib, "hostile", mode, recompute, B, H, W, 0xFF, True, channels_last=1)
    assert torch.equal(d_cl, res[True, 0x00][0])


@pytest.mark.parametrize("mode", ah.TRAIN_MODES)
def test_abi_embed_px_so400m_1layer_384(pkg, hiplib, mode):
    d0, _ = _abi_input_gradient(pkg, hiplib, "so400m-1layer", mode, 0, 1, 384, 384, 0x00, True)
    d1, _ = _abi_input_gradient(pkg, hiplib, "so400m-1layer", mode, 0, 1, 384, 384, 0xFF, True)
    assert bool(torch.isfinite(d0).all()) and torch.equal(d0, d1) and d0.abs().max().item() > 0
    assert border_is_zero(d0, 14)                                             # 384 = 27 * 14 + 6


# ---- 8. surfaces -------------------------------------------------------------------------------------------------
def test_encode_image_input_gradient_vs_oracle(pkg, oracle, hiplib):
    cfg = pkg.get_config("hostile")
    sd = pkg.weights.seeded_state_dict(cfg, seed=31)
    enc = pkg.OpenClipStyleEncoder(cfg, "fp32")
    enc.visual.load_state_dict(sd)
    enc = enc.cuda().requires_grad_(False)
    x_cpu = pkg.weights.seeded_pixels(2, 42, 42, seed=1031)
    x = x_cpu.cuda().requires_grad_(True)
    f = enc.encode_image(x, normalize=True)
    w = torch.cos(torch.arange(f.numel(), dtype=torch.float32) * 0.37 + 0.11).reshape(f.shape)
    (f * w.cuda()).sum().backward()
    xr = x_cpu.clone().requires_grad_(True)
    fr = oracle.vision_forward(xr, sd, cfg, False, False)["pooler_output"]
    fr = fr / fr.norm(dim=-1, keepdim=True)
    (fr * w).sum().backward()
    err, bar = (x.grad.cpu() - xr.grad).abs().max().item(), strict_bar(xr.grad.abs().max().item(), "fp32")
    print(f"[encode_image/fp32] d_pixels vs oracle max|err| {err:.3e} (bar {bar:.3e})")
    assert err <= bar and all(p.grad is None for p in enc.parameters())


def test_image_binary_classifier_frozen_bce_input_gradient_vs_oracle(pkg, oracle, hiplib):
    """The attack step: frozen detector, BCE on its logit, gradient w.r.t. the image (FGSM's sign(d_pixels))."""
    cfg = pkg.get_config("hostile")
    sd = pkg.weights.seeded_state_dict(cfg, seed=32)
    enc = pkg.OpenClipStyleEncoder(cfg, "fp32")
    enc.visual.load_state_dict(sd)
    torch.manual_seed(5)
    clf = pkg.heads.ImageBinaryClassifierHIP(enc)
    head_cpu = copy.deepcopy(clf.head).eval()
    clf = clf.cuda().eval().requires_grad_(False)
    x_cpu = pkg.weights.seeded_pixels(3, 42, 42, seed=1032)
    y = torch.tensor([1.0, 0.0, 1.0])
    x = x_cpu.cuda().requires_grad_(True)
    loss = torch.nn.functional.binary_cross_entropy_with_logits(clf(x), y.cuda())
    loss.backward()
    xr = x_cpu.clone().requires_grad_(True)
    logit = head_cpu(oracle.vision_forward(xr, sd, cfg, False, False)["pooler_output"])
    lr = torch.nn.functional.binary_cross_entropy_with_logits(logit, y)
    lr.backward()
    err, bar = (x.grad.cpu() - xr.grad).abs().max().item(), strict_bar(xr.grad.abs().max().item(), "fp32")
    print(f"[ImageBinaryClassifierHIP/fp32] loss {loss.item():.6f} vs {lr.item():.6f}; d_pixels max|err| {err:.3e} "
          f"(bar {bar:.3e}, max|ref| {xr.grad.abs().max().item():.3e})")
    assert abs(loss.item() - lr.item()) <= 2e-5 * max(1.0, abs(lr.item()))
    assert err <= bar and all(p.grad is None for p in clf.parameters())
    x_adv = (x + 0.01 * x.grad.sign()).detach()                                # FGSM raises the loss it ascends
    assert torch.nn.functional.binary_cross_entropy_with_logits(clf(x_adv), y.cuda()).item() > loss.item()


@pytest.mark.parametrize("wrapper", ["fast_binary", "mtl"])
def test_other_wrappers_return_an_input_gradient(wrapper, pkg, hiplib):
    cfg = pkg.get_config("tiny")
    sd = pkg.weights.seeded_state_dict(cfg, seed=33)
    torch.manual_seed(6)
    x = pkg.weights.seeded_pixels(2, 32, 32, seed=1033).cuda().requires_grad_(True)
    if wrapper == "fast_binary":
        enc = pkg.OpenClipStyleEncoder(cfg, "bf16")
        enc.visual.load_state_dict(sd)
        model = pkg.heads.FastBinaryClassifierHIP(enc).cuda().eval().requires_grad_(False)
        loss = model(x).float().sum()
    else:
        cfg = pkg.get_config("hostile")
        enc = pkg.SiglipVisionModelHIP(cfg, "fp32")
        enc.load_state_dict(pkg.weights.seeded_state_dict(cfg, seed=33))
        model = pkg.heads.SigLIP2MTL(enc, seg_layers=(0, 1, -1), embed_dim=32, freeze_below=1).cuda().eval()
        x = pkg.weights.seeded_pixels(3, 56, 56, seed=1033).cuda().requires_grad_(True)
        cls_logit, seg = model(x)
        loss = cls_logit.float().square().sum() + seg.float().mean()           # saliency of the mask logits included
    loss.backward()
    assert x.grad is not None and x.grad.shape == x.shape and bool(torch.isfinite(x.grad).all())
    assert x.grad.abs().max().item() > 0


# ---- 9. full depth -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_full_depth_so400m_384_frozen(mode, pkg, hiplib):
    rec = pg.load(pg.FULL_CASE)
    _, d, grads, model = case_run(pkg, rec, mode, frozen=True)
    assert not grads and bool(torch.isfinite(d).all()) and border_is_zero(d, 14)
    check_against_fixture(rec, mode, d, pg.FULL_CASE, maxerr_bar=False)        # 16-bit modes: the rel-L2 bar only


# ---- 10. refusals ------------------------------------------------------------------------------------------------
def test_refusals_say_what_to_do_instead(pkg, hiplib):
    """What stays unsupported raises a RuntimeError that names the limit (no silent wrong gradient)."""
    x = pkg.weights.seeded_pixels(2, 32, 32, seed=4).cuda()
    model = build(pkg, "tiny", 3, "bf16")
    patches = pkg.preprocess.to_patch_operand(x * 0.5 + 0.5, model.config, compute_dtype="bf16")
    patches.data.requires_grad_(True)
    with pytest.raises(RuntimeError, match="differentia"):          # layout 2: the fused input transform
        model(patches=patches)
    mx = build(pkg, "tiny", 3, "mxfp8").requires_grad_(False)
    with pytest.raises(RuntimeError, match="differentia"):          # inference-only mode
        mx(pixel_values=x.clone().requires_grad_(True))
    xg = x.clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="differentia"):          # double backward
        out = model(pixel_values=xg)
        torch.autograd.grad(out.pooler_output.square().sum(), xg, create_graph=True)
