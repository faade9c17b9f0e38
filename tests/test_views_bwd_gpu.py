"""GPU: sgl_op_preprocess_views_bwd, the adjoint of the app's test-time views with respect to a float source, through the
C ABI and up to `x.grad` of `heads.app_visual_prob` over the encoder.

The discipline of tests/test_preprocess_bwd_gpu.py: every element of d_src is held to its own derived bound against the
float64 reference of tests/views_bwd_ref.py (asserted on the CPU in tests/test_views_bwd_host.py), d_src sits between
sentinel guard rows with a NaN body, each case is named after the branch it is there for and prints its worst err/bound
as a RATIO line before it asserts, and refusals write nothing.  The view sets live in tests/views_bwd_ref.py:
orientation (40 overlapping views: every turn, exact and on the kept canvas, for w - h odd, even and zero, the mirror
alone and after a turn), the five scale boxes and the copy shortcut turned and mirrored, coverage (an image without a
view, a border no box holds, a pixel nine views hold), 64 / 65 / 130 records (one launch, two, three), the app's 42 + 2.
"""
import copy

import pytest
import torch

import kernel_ref as kr
import preprocess_bwd_ref as pb
import views_bwd_ref as vb
import views_ref as vr
from kernel_ref import F32
from test_input_grad_gpu import build, strict_bar
from test_kernel_edges_aux_gpu import BAD_SHAPE, NULL, UNSUPPORTED, WORKSPACE, untouched, within
from test_kernel_edges_gpu import DEV, Guarded, P, lib, ok, stream  # noqa: F401  (lib: fixture)

pytestmark = pytest.mark.gpu


def table(pkg, views):
    """ctypes sgl_view[V] of plain (src, box, turns, keep_canvas, flip) tuples, unchecked (refusals need bad ones)."""
    return (pkg.lib.SglView * len(views))(*(pkg.lib.SglView(b, *box, t, int(k), int(f)) for b, box, t, k, f in views))


def run_bwd(pkg, lib, G_d, B, Hs, Ws, views, S, std, out):
    tab = table(pkg, views)
    n = lib.sgl_op_preprocess_views_bwd_scratch_bytes(tab, len(views), S)
    scratch = torch.empty(n, device=DEV, dtype=torch.uint8) if n else None
    st = lib.sgl_op_preprocess_views_bwd(P(G_d), B, Hs, Ws, tab, len(views), S, std, out.ptr, P(scratch), n, stream())
    torch.cuda.synchronize()                             # scratch stays alive until the kernels have run
    return st


def d_src_of(pkg, lib, name, std=0.5, what=None):
    """One call of a named case on a guarded, poisoned d_src: (got (B,3,Hs,Ws) on the device, the case's reference)."""
    case = vb.case_reference(pkg.preprocess, name, std)
    B, Hs, Ws, S, views, G = case[:6]
    out = Guarded(B * 3 * Hs, Ws, Ws, torch.float32)
    ok(run_bwd(pkg, lib, G.to(DEV), B, Hs, Ws, views, S, std, out))
    out.check(what or name)
    return out.got().view(B, 3, Hs, Ws), case


@pytest.mark.parametrize("std", [0.5, 0.25])
@pytest.mark.parametrize("name", vb.CASE_NAMES)
def test_views_bwd_cases(pkg, lib, name, std):
    what = f"views_bwd {name} std{std}"
    got, (B, Hs, Ws, S, views, G, ref, bound, n) = d_src_of(pkg, lib, name, std, what)
    within(got, ref, bound, what)
    nobody = (n == 0)[:, None].expand(B, 3, Hs, Ws)
    assert bool((got.cpu().view(torch.int32)[nobody] == 0).all()), f"{what}: an element no view reaches is not +0.0"
    if name == "coverage":
        y, x = vb.COVER_PIXEL
        assert n[0, y, x] >= 8 and bool((n[2] == 0).all()) and int(nobody.sum()) > 3 * Hs * Ws
        assert bool((got[2].cpu().view(torch.int32) == 0).all())              # the image no view names: bit for bit zero


def test_views_bwd_grid_stride(pkg, lib):
    """2 x 1040 x 1040: 8450 tiles of 16 x 16 pixels for the 8192 blocks of the capped grid, so the last 258 tiles (the
    bottom rows of image 1, under three of the views) are a block's second trip."""
    got, (B, Hs, Ws, S, views, G, ref, bound, n) = d_src_of(pkg, lib, "grid_stride")
    assert B * ((Hs + 15) // 16) * ((Ws + 15) // 16) > 8192
    within(got, ref, bound, "views_bwd grid_stride")


@pytest.mark.parametrize("name", ["orientation", "chunk_V130", "app"])
def test_views_bwd_is_bitwise_reproducible(pkg, lib, name):
    a, _ = d_src_of(pkg, lib, name)
    b, _ = d_src_of(pkg, lib, name)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("name", ["orientation", "app"])
def test_adjoint_identity_with_the_forward_kernel(pkg, lib, name):
    """<views(x), G> = <x, views_bwd(G)> with mean = 0, both dot products in float64, independent of the backward's
    reference: each side is off by at most its kernel's error against the exact operator, sum|G| bound_fwd on the left
    (tests/views_ref.py), sum|x| bound_bwd on the right."""
    std = 0.5
    got, (B, Hs, Ws, S, views, G, _, bound_bwd, _) = d_src_of(pkg, lib, name, std)
    x = kr.image_source(B, Hs, Ws, False, seed=61)
    V = len(views)
    fwd = Guarded(V * 3 * S, S, S, torch.float32)
    x_d = x.to(DEV)
    ok(lib.sgl_op_preprocess_views(P(x_d), 0, B, Hs, Ws, table(pkg, views), V, fwd.ptr, F32, S, 14, 640, 0, 0.0, std, None,
                                   0, stream()))
    torch.cuda.synchronize()
    fwd.check(name)
    _, bound_fwd = vr.views_ref(x, False, views, S, 14, 640, False, 0.0, std, torch.float32)
    lhs = (fwd.got().view(V, 3, S, S).cpu().double() * G.double()).sum().item()
    rhs = (x.double() * got.cpu().double()).sum().item()
    slack = ((G.double().abs() * bound_fwd).sum() + (x.double().abs() * bound_bwd).sum()).item()
    print(f"RATIO adjoint_identity {abs(lhs - rhs) / slack:.3e}  {name}: <Ax, G> {lhs:.9g} <x, A^T G> {rhs:.9g} slack {slack:.3g}")
    assert abs(lhs - rhs) <= slack


def test_views_bwd_refusals_write_nothing(pkg, lib):
    B, Hs, Ws, S = 2, 60, 230, 14
    good = [(1, (3, 5, 53, 35), 1, False, True), (0, (10, 4, 24, 18), 0, False, False)]     # 50 x 30 turned; a 14 x 14 copy
    G_d = vb.grad_input(2, S, seed=4).to(DEV)
    out = Guarded(B * 3 * Hs, Ws, Ws, torch.float32)
    need = lib.sgl_op_preprocess_views_bwd_scratch_bytes(table(pkg, good), 2, S)
    assert need == 2 * S * 20 + (50 + 30) * 8
    scratch = torch.empty(need, device=DEV, dtype=torch.uint8)

    def call(g=G_d, Bn=B, Hs_=Hs, Ws_=Ws, rec=good[1], V=2, S_=S, std=0.5, dst=out.ptr, sc=scratch, nb=need, tab="table"):
        t = table(pkg, [good[0], rec]) if tab == "table" else tab
        return lib.sgl_op_preprocess_views_bwd(P(g), Bn, Hs_, Ws_, t, V, S_, std, dst, P(sc), nb, stream())
    assert call(g=None) == NULL and call(dst=None) == NULL and call(tab=None) == NULL and call(sc=None) == NULL
    assert call(V=0) == BAD_SHAPE and call(Bn=0) == BAD_SHAPE and call(Hs_=0) == BAD_SHAPE and call(Ws_=0) == BAD_SHAPE
    assert call(S_=0) == BAD_SHAPE and call(std=0.0) == BAD_SHAPE and call(Bn=1) == BAD_SHAPE
    for rec in ((2, (0, 0, 50, 40), 0, 0, 0), (0, (-1, 0, 50, 40), 0, 0, 0), (0, (50, 0, 50, 40), 0, 0, 0),
                (0, (0, 0, 231, 40), 0, 0, 0), (0, (0, 0, 50, 61), 0, 0, 0), (0, (0, 0, 50, 40), 4, 0, 0),
                (0, (0, 0, 50, 40), 0, 2, 0), (0, (0, 0, 50, 40), 0, 0, 2)):
        assert call(rec=rec) == BAD_SHAPE, rec            # the first record is a good one: nothing of it is written either
    assert call(rec=(0, (0, 0, 225, 40), 0, 0, 0)) == UNSUPPORTED            # 225 / 14 = 16.07
    assert call(rec=(0, (0, 0, 225, 40), 1, 0, 0)) == UNSUPPORTED            # the same extent turned onto the y axis
    assert call(nb=need - 1) == WORKSPACE and call(nb=0) == WORKSPACE
    torch.cuda.synchronize()
    untouched(out, "views_bwd refusals")


# ---- autograd ----------------------------------------------------------------------------------------------------
def app_view_objects(pp, h, w):
    return [pp.View(b, box, t, k, f) for b, box, t, k, f in vb.app_views(pp, h, w)]


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16], ids=["f32out", "bf16out"])
def test_views_resize_normalize_autograd(pkg, lib, out_dtype):
    pp = pkg.preprocess
    B, Hs, Ws, S, views, _, _, _, _ = vb.case_reference(pp, "app", 0.25)
    objs = app_view_objects(pp, Hs, Ws)
    V = len(objs)
    src = kr.image_source(B, Hs, Ws, False, seed=62).to(DEV)
    x = src.clone().requires_grad_(True)
    y = pp.views_resize_normalize(x, objs, S, 0.5, 0.25, dtype=out_dtype, differentiable=True)
    y0 = pp.views_resize_normalize(src, objs, S, 0.5, 0.25, dtype=out_dtype)                # the default call
    assert y.requires_grad and y.grad_fn is not None and not y0.requires_grad
    assert torch.equal(y.detach(), y0) and y.dtype == out_dtype and y.shape == (V, 3, S, S)
    assert not pp.views_resize_normalize(src, objs, S, differentiable=True).requires_grad   # nothing to differentiate
    with torch.no_grad():
        assert not pp.views_resize_normalize(x, objs, S, differentiable=True).requires_grad
    G = vb.grad_input(V, S, seed=63).to(out_dtype)
    y.backward(G.to(DEV))
    assert x.grad.dtype == torch.float32 and x.grad.shape == x.shape
    vjp = pp.views_resize_normalize_backward(G.to(DEV), objs, (B, Hs, Ws), std=0.25)
    assert vjp.dtype == torch.float32 and torch.equal(x.grad, vjp)
    ref, bound, _ = vb.views_bwd_ref(G.float(), views, B, Hs, Ws, S, 0.25)
    within(x.grad, ref, bound, f"views_autograd x.grad {out_dtype}")


@pytest.mark.parametrize("kind", ["fp16", "bf16", "channels_last", "strided"])
def test_views_autograd_source_layouts(pkg, lib, kind):
    """The gradient comes back in the source's dtype and shape; a 16-bit source gets the fp32 gradient rounded once."""
    pp = pkg.preprocess
    B, Hs, Ws, S = 2, 30, 37, 42
    views = [pp.View(b, box, t, k, f) for b, box, t, k, f in vb.random_views(7, B, Hs, Ws, seed=64)]
    src = kr.image_source(B, Hs + 2, Ws, False, seed=65).to(DEV)
    if kind in ("fp16", "bf16"):
        x = src[:, :, :Hs].to(torch.float16 if kind == "fp16" else torch.bfloat16)
    elif kind == "channels_last":
        x = src[:, :, :Hs].contiguous(memory_format=torch.channels_last)
    else:
        x = src[:, :, 1:Hs + 1]                            # a non-contiguous view
        assert not x.is_contiguous()
    x = x.detach().requires_grad_(True)
    y = pp.views_resize_normalize(x, views, S, differentiable=True)
    assert torch.equal(y.detach(), pp.views_resize_normalize(x.detach(), views, S))
    G = vb.grad_input(len(views), S, seed=66).to(DEV)
    y.backward(G)
    want = pp.views_resize_normalize_backward(G, views, (B, Hs, Ws))
    assert x.grad.dtype == x.dtype and x.grad.shape == x.shape
    assert torch.equal(x.grad, want.to(x.dtype))


def test_backward_for_a_uint8_source_is_the_float_path_on_bytes_over_255(pkg, lib):
    pp = pkg.preprocess
    B, Hs, Ws, S = 2, 40, 33, 32
    views = [pp.View(b, box, t, k, f) for b, box, t, k, f in vb.random_views(6, B, Hs, Ws, seed=67)]
    u8 = kr.image_source(B, Hs, Ws, True, seed=68).to(DEV)                     # NHWC bytes
    G = vb.grad_input(len(views), S, seed=69).to(DEV)
    assert not pp.views_resize_normalize(u8, views, S, differentiable=True).requires_grad
    xf = (u8.permute(0, 3, 1, 2).float() / 255.0).requires_grad_(True)
    pp.views_resize_normalize(xf, views, S, differentiable=True).backward(G)
    assert torch.equal(pp.views_resize_normalize_backward(G, views, (B, Hs, Ws)), xf.grad)
    with pytest.raises(ValueError, match="rows"):
        pp.views_resize_normalize_backward(G[:-1], views, (B, Hs, Ws))


def test_double_backward_raises_and_the_other_routes_still_refuse(pkg, lib):
    pp = pkg.preprocess
    cfg = pkg.get_config("tiny")
    src = kr.image_source(1, 40, 40, False, seed=70).to(DEV)
    x = src.clone().requires_grad_(True)
    views, _ = pp.multicrop_views(40, 40)
    y = pp.views_resize_normalize(x, views, 32, differentiable=True)
    (g,) = torch.autograd.grad(y.square().sum(), x, create_graph=True)        # grad_out = 2 y carries a graph
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()
    with pytest.raises(RuntimeError, match="differentia") as e:
        pp.views_resize_normalize(x, views, 32)
    assert "differentiable=True" in str(e.value)
    with pytest.raises(RuntimeError, match="differentia") as e:
        pp.views_to_patch_operand(x, views, cfg, size=32)
    assert "views_resize_normalize" in str(e.value) and "differentiable=True" in str(e.value) and "pixel_values=" in str(e.value)


# ---- end to end --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_source_gradient_of_the_app_visual_probability(pkg, oracle, lib, mode):
    """x -> 42 views -> model(pixel_values=) -> linear head -> app_visual_prob.  The method of
    tests/test_preprocess_bwd_gpu.py::test_source_gradient_through_the_encoder: d_pixels itself is pinned to HF by
    tests/test_input_grad_gpu.py in every mode, so what is left is the chain rule, x.grad bitwise the VJP of p.grad, and
    that asking for the source gradient moves no bit of the logits.  In fp32 x.grad is also held to the CPU oracle (the
    oracle encoder behind torch's float64 autograd of the views) under the bar that file holds fp32 d_pixels to against
    the oracle, 1e-7 + 6e-5 max|ref|; the bf16 figure is printed."""
    pp, H = pkg.preprocess, pkg.heads
    cfg = pkg.get_config("tiny")
    S = cfg.image_size
    model = build(pkg, "tiny", 3, mode).eval().requires_grad_(False)
    torch.manual_seed(11)
    head_cpu = torch.nn.Linear(cfg.hidden_size, 1)
    head = copy.deepcopy(head_cpu).to(DEV).requires_grad_(False)
    h, w = 70, 97
    d = pp.detect_views(h, w)
    assert len(d.views) == 42
    src = kr.image_source(1, h, w, False, seed=71)

    def prob_of(px):
        return H.app_visual_prob(head(model(pixel_values=px).pooler_output.float()).squeeze(-1), d)

    x = src.to(DEV).requires_grad_(True)
    prob_a = prob_of(pp.views_resize_normalize(x, d.views, S, differentiable=True))
    prob_a.backward()
    p = pp.views_resize_normalize(src.to(DEV), d.views, S).requires_grad_(True)
    prob_b = prob_of(p)
    prob_b.backward()
    assert torch.equal(prob_a, prob_b)                                         # asking for the source gradient moves nothing
    assert x.grad is not None and x.grad.shape == x.shape and x.grad.abs().max().item() > 0
    assert torch.equal(x.grad, pp.views_resize_normalize_backward(p.grad, d.views, (1, h, w)))
    sd = pkg.weights.seeded_state_dict(cfg, seed=3)
    xr = src.double().requires_grad_(True)
    pooled = oracle.vision_forward(vb.torch_views(xr, d.views, S, 0.5, 0.5).float(), sd, cfg, False, False)["pooler_output"]
    prob_r = H.app_visual_prob(head_cpu(pooled).squeeze(-1), d)
    prob_r.backward()
    err = (x.grad.cpu().double() - xr.grad).abs().max().item()
    bar = strict_bar(xr.grad.abs().max().item(), "fp32")
    print(f"[app_visual_prob/{mode}] p {prob_a.item():.6f} vs oracle {prob_r.item():.6f}; x.grad max|err| {err:.3e} "
          f"(fp32 bar {bar:.3e}, {err / bar:.2f} of it; max|ref| {xr.grad.abs().max().item():.3e})")
    if mode == "fp32":
        assert abs(prob_a.item() - prob_r.item()) <= 2e-5
        assert err <= bar
        x_adv = (src.to(DEV) + 0.01 * x.grad.sign()).detach()                  # one FGSM step on the SOURCE raises the verdict
        with torch.no_grad():
            assert prob_of(pp.views_resize_normalize(x_adv, d.views, S)).item() > prob_a.item()
