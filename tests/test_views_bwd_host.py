"""CPU (no GPU): the reference of the view transform's adjoint (tests/views_bwd_ref.py), the C ABI's refusals and
`heads.app_visual_prob`.

* the float64 reference (per-view `preprocess_bwd_ref` on the oriented image, moved back through the inverse of
  `views_ref.orient`, added into the box) equals torch's own float64 autograd of crop -> orient -> F.interpolate(bilinear,
  antialias=True) -> normalise, summed over the views, to 1e-12 on unit-variance G, on every view set of the GPU tests;
* torch's fp32 backward of the same graph stays inside the derived bound with worst ratio <= 0.5, the rule
  tests/test_preprocess_bwd_host.py holds fp32 evaluations to;
* the bound catches three mutants: a covering view left out at a pixel, the kept canvas indexed with truncation toward
  zero instead of the `>> 1` floor, and the mirror applied before the turn instead of after it;
* sgl_op_preprocess_views_bwd / sgl_op_preprocess_views_bwd_scratch_bytes exist and every documented argument error
  returns its code before the first HIP call (dummy pointers, no launch: the method of tests/test_abi_aux_host.py);
* `app_visual_prob` is the `visual_prob` of `core_signals_batched` and passes torch's gradcheck in float64.
"""
import pytest
import torch

import kernel_ref as kr
import views_bwd_ref as vb
import views_ref as vr

OK, BAD_SHAPE, UNSUPPORTED, WORKSPACE, NULL = 0, -1, -2, -3, -5
D = 0x7F0000001000          # a 16-byte aligned dummy device pointer, never dereferenced


@pytest.mark.parametrize("name", vb.CASE_NAMES)
def test_reference_equals_torch_float64_autograd(pkg, name):
    for std in (0.5, 0.25):
        B, Hs, Ws, S, views, G, ref, _, _ = vb.case_reference(pkg.preprocess, name, std)
        want = vb.torch_autograd(G, views, B, Hs, Ws, S, std)
        err = (ref - want).abs().max().item()
        print(f"REFERR {name} std {std}: {err:.3e}")
        assert tuple(ref.shape) == (B, 3, Hs, Ws)
        assert err <= 1e-12


@pytest.mark.parametrize("name", vb.CASE_NAMES)
def test_torch_fp32_backward_stays_inside_half_the_bound(pkg, name):
    """Measured worst ratios (pytest -rP prints every case): 0.14 on the copy shortcut with a turn and a mirror, where the
    adds over the views are all there is, 0.12 at V = 130 (43 views on one pixel), 0.08 or less on the other sets."""
    for std in (0.5, 0.25):
        B, Hs, Ws, S, views, G, ref, bound, n = vb.case_reference(pkg.preprocess, name, std)
        assert bool((bound > 0).all())
        got = vb.torch_autograd(G, views, B, Hs, Ws, S, std, dtype=torch.float32)
        r = kr.assert_within(got, ref, bound, f"torch fp32 backward {name} std {std}")
        print(f"RATIO {name} std {std}: torch-fp32 {r:.4f} (most views on one pixel: {int(n.max().item())})")
        assert r <= 0.5
        assert bool((got[(n == 0)[:, None].expand_as(got)] == 0).all())      # what no view reaches is exactly zero


def test_coverage_case_has_an_unviewed_image_a_border_and_a_crowded_pixel(pkg):
    B, Hs, Ws, S, views, G, ref, bound, n = vb.case_reference(pkg.preprocess, "coverage")
    y, x = vb.COVER_PIXEL
    assert n[0, y, x] >= 8 and bool((n[2] == 0).all()) and bool((n[0, :3] == 0).all()) and bool((n[1, :2] == 0).all())
    assert bool((ref[2] == 0).all()) and bool((bound[2] == kr.TINY[torch.float32]).all())


def test_bound_catches_a_view_left_out_at_a_pixel(pkg):
    """At the crowded pixel of the coverage set, every one of its views in turn: the sum without that view's term."""
    B, Hs, Ws, S, views, G, ref, bound, n = vb.case_reference(pkg.preprocess, "coverage")
    y, x = vb.COVER_PIXEL
    terms = vb.view_terms(G, views, S)
    left_out = 0
    for b, (x0, y0, x1, y1), Fc, _, hit in terms:
        if b != 0 or not (x0 <= x < x1 and y0 <= y < y1) or not hit[y - y0, x - x0]:
            continue
        mutant = ref.clone()
        mutant[0, :, y, x] -= Fc[:, y - y0, x - x0] / 0.5
        r = kr.worst_ratio(mutant, ref, bound)
        print(f"MUTANT view left out, box {(x0, y0, x1, y1)}: ratio {r:.3e}")
        assert r > 100
        left_out += 1
    assert left_out >= 8


def _orient_truncating(C, turns, keep, flip):
    """`views_ref.orient` with the kept canvas indexed by truncation toward zero where the rule floors (`>> 1`)."""
    if not (keep and turns in (1, 3)):
        return vr.orient(C, turns, keep, flip)
    h, w = C.shape[-2:]
    half = lambda a: int(a / 2)                            # noqa: E731  (toward zero; a >> 1 floors)
    y, x = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    if turns == 1:
        cx, cy = half(w + h - 1) - y, half(h - w + 1) + x
    else:
        cx, cy = half(w - h + 1) + y, half(w + h - 1) - x
    inside = (cx >= 0) & (cx < w) & (cy >= 0) & (cy < h)
    O = torch.where(inside, C[..., cy.clamp(0, h - 1), cx.clamp(0, w - 1)], torch.zeros((), dtype=C.dtype))
    return O.flip(-1) if flip else O


def _orient_flip_first(C, turns, keep, flip):
    return vr.orient(C.flip(-1) if flip else C, turns, keep, False)


def test_bound_catches_a_truncating_kept_canvas_and_a_mirror_before_the_turn(pkg):
    """Both on the orientation set as a whole, and view by view on the views the mutation can reach.

    The floor differs from truncation only for a negative odd numerator: h - w + 1 at one turn (w > h + 1), w - h + 1 at
    three turns (h > w + 1), and odd only when w - h is EVEN (w + h - 1 is positive).  So it is the 50 x 34 box where this
    mutant is off by one; for w - h odd (51 x 34, 34 x 51) both numerators are even, no rounding happens, and the mutant is
    the rule itself: asserted below, so that nobody looks for an off-by-one there."""
    B, Hs, Ws, S, views, G, ref, bound, _ = vb.case_reference(pkg.preprocess, "orientation")
    for what, orient in (("truncating kept canvas", _orient_truncating), ("mirror before the turn", _orient_flip_first)):
        mutant = vb.torch_autograd(G, views, B, Hs, Ws, S, 0.5, orient=orient)
        r = kr.worst_ratio(mutant, ref, bound)
        print(f"MUTANT {what}, 40 views: ratio {r:.3e}")
        assert r > 100
    for v, view in enumerate(views):
        _, box, turns, keep, flip = view
        w, h = box[2] - box[0], box[3] - box[1]
        one_ref, one_bound, _ = vb.views_bwd_ref(G[v:v + 1], [view], B, Hs, Ws, S, 0.5)
        r_trunc = kr.worst_ratio(vb.torch_autograd(G[v:v + 1], [view], B, Hs, Ws, S, 0.5, orient=_orient_truncating),
                                 one_ref, one_bound)
        r_flip = kr.worst_ratio(vb.torch_autograd(G[v:v + 1], [view], B, Hs, Ws, S, 0.5, orient=_orient_flip_first),
                                one_ref, one_bound)
        bites = keep and ((turns == 1 and w > h + 1) or (turns == 3 and h > w + 1)) and (w - h) % 2 == 0
        assert (r_trunc > 100) if bites else (r_trunc <= 0.5), (view, r_trunc)
        assert (r_flip > 100) if (flip and turns % 2 == 1) else (r_flip <= 0.5), (view, r_flip)
    assert sum(1 for _, b, t, k, f in views if k and t == 1 and (b[2] - b[0] - b[3] + b[1]) % 2 == 0 and b[2] - b[0] > b[3] - b[1]) >= 2


def test_symbols_exist_and_argument_errors_return_before_any_launch(pkg, hiplib):
    lib = hiplib
    declared = pkg.lib.declared_symbols()
    for s in ("sgl_op_preprocess_views_bwd", "sgl_op_preprocess_views_bwd_scratch_bytes"):
        assert s in declared, s
        assert getattr(lib, s).argtypes is not None, s
    assert lib.sgl_abi_version() == 3                               # new symbols only

    def table(views):
        return (pkg.lib.SglView * len(views))(*(pkg.lib.SglView(b, *box, t, int(k), int(f)) for b, box, t, k, f in views))
    good = [(1, (3, 5, 53, 35), 1, False, True), (0, (10, 4, 52, 46), 0, False, False)]     # 50 x 30 turned; a 42 x 42 copy
    need = lib.sgl_op_preprocess_views_bwd_scratch_bytes(table(good), 2, 42)
    assert need == 2 * 42 * 20 + (50 + 30) * 8                      # two filter tables, two span tables; the copy needs none
    assert lib.sgl_op_preprocess_views_bwd_scratch_bytes(table(good[1:]), 1, 42) == 0
    assert lib.sgl_op_preprocess_views_bwd_scratch_bytes(None, 2, 42) == 0
    assert lib.sgl_op_preprocess_views_bwd_scratch_bytes(table(good), 0, 42) == 0
    app = vb.app_views(pkg.preprocess, 1024, 1024)[:42]
    mb = lib.sgl_op_preprocess_views_bwd_scratch_bytes(table(app), 42, 384) / 1e6
    print(f"SCRATCH 42 views of 1024 x 1024 at S = 384: {mb:.3f} MB")
    assert 0.5 < mb < 1.5

    def call(d_out=D, Bn=2, Hs=60, Ws=70, rec=good[1], V=2, S=42, std=0.5, d_src=D, scratch=D, nbytes=need, tab="table"):
        t = table([good[0], rec]) if tab == "table" else tab
        return lib.sgl_op_preprocess_views_bwd(d_out, Bn, Hs, Ws, t, V, S, std, d_src, scratch, nbytes, None)
    assert call(d_out=None) == NULL and call(d_src=None) == NULL and call(tab=None) == NULL
    assert call(d_out=None, V=0) == NULL                            # pointers are checked first
    assert call(std=0.0) == BAD_SHAPE
    for over in (dict(V=0), dict(V=-1), dict(Bn=0), dict(Hs=0), dict(Ws=0), dict(S=0), dict(Bn=1)):    # Bn=1: src 1 outside
        assert call(**over) == BAD_SHAPE, over
    for rec in ((2, (0, 0, 50, 40), 0, 0, 0), (-1, (0, 0, 50, 40), 0, 0, 0), (0, (-1, 0, 50, 40), 0, 0, 0),
                (0, (50, 0, 50, 40), 0, 0, 0), (0, (0, 0, 71, 40), 0, 0, 0), (0, (0, 0, 50, 61), 0, 0, 0),
                (0, (0, 7, 50, 7), 0, 0, 0), (0, (0, 0, 50, 40), 4, 0, 0), (0, (0, 0, 50, 40), -1, 0, 0),
                (0, (0, 0, 50, 40), 0, 2, 0), (0, (0, 0, 50, 40), 0, 0, 2)):
        assert call(rec=rec) == BAD_SHAPE, rec
    wide = (0, (0, 0, 225, 40), 0, 0, 0)                            # 225 / 14 = 16.07
    assert call(Ws=230, S=14, rec=wide) == UNSUPPORTED
    assert call(Ws=230, S=14, rec=(0, (0, 0, 225, 40), 1, 0, 0)) == UNSUPPORTED      # the same extent turned onto the y axis
    assert call(Ws=230, S=14, rec=(0, (0, 0, 224, 40), 0, 0, 0), nbytes=0) == WORKSPACE     # exactly 16x is admitted
    assert call(nbytes=need - 1) == WORKSPACE and call(nbytes=0) == WORKSPACE
    assert call(scratch=None) == NULL                               # bytes are needed here
    assert call(rec=wide, Ws=230, S=14, scratch=None, nbytes=0) == UNSUPPORTED      # the records are judged before the scratch


def test_app_visual_prob_is_core_signals_visual_prob_and_differentiable(pkg):
    H, pp = pkg.heads, pkg.preprocess
    d = pp.detect_views(70, 97)
    g = torch.Generator().manual_seed(7)
    z = torch.randn(len(d.views), generator=g) * 2.0
    fusion = torch.nn.Linear(2, 1)
    want = H.core_signals_batched(z[d.crops][None], d.weights, torch.zeros(1, 9), z[d.rot][None], fusion,
                                  H.CoralCalibrator())["visual_prob"]
    got = H.app_visual_prob(z, d)
    assert got.shape == want.shape == (1,) and torch.equal(got, want)
    restated = 0.6 * torch.sigmoid((z[:9].double() * d.weights.double()).sum()) + 0.4 * torch.sigmoid(z[9].double())
    assert abs(got.item() - restated.item()) <= 1e-6
    zr = z.clone().requires_grad_(True)
    H.app_visual_prob(zr, d).backward()
    assert bool((zr.grad[:10] != 0).all()) and bool((zr.grad[10:] == 0).all())      # crops and the rotated frame only
    z64 = z.double().requires_grad_(True)
    assert H.app_visual_prob(z64, d).dtype == torch.float64
    assert torch.autograd.gradcheck(lambda t: H.app_visual_prob(t, d), (z64,))


def test_python_surface_names_the_differentiable_route(pkg):
    """CPU part of the Python surface: the signature, the VJP's argument checks and the CUDA-only rule."""
    import inspect
    pp = pkg.preprocess
    assert inspect.signature(pp.views_resize_normalize).parameters["differentiable"].default is False
    views = [pp.View(0, (0, 0, 30, 20))]
    with pytest.raises(RuntimeError, match="CUDA tensors only"):
        pp.views_resize_normalize_backward(torch.zeros(1, 3, 8, 8), views, (1, 20, 30))
    with pytest.raises(RuntimeError, match="CUDA tensors only"):
        pp.views_resize_normalize(torch.zeros(1, 3, 20, 30, requires_grad=True), views, 8, differentiable=True)
