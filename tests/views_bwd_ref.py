"""float64 reference and per-element bound for sgl_op_preprocess_views_bwd (csrc/preprocess.hip), the adjoint of the
app's test-time views (crop -> quarter turn -> mirror -> Resize(S, antialias=True) -> Normalize) with respect to a float
source, and the view sets its CPU and GPU tests share.

By the conventions at the top of tests/kernel_ref.py: the reference is the same operation in float64 on the fp32 gradient
the kernel received; the bound is per element and derived, not fitted.

    F_v      = Wy_v^T G[v] Wx_v                                the filter sum of view v on its ORIENTED image (oh x ow):
                                                               `preprocess_bwd_ref(G[v], oh, ow, S, 1.0, None, 1.0)`
    d_src[b] = (sum over {v : src_v = b} of unorient_v(F_v) placed at box_v) / std

  per view  `preprocess_bwd_ref` bounds the kernel's `bwd_filter_sum` element by element (the weights' errors and the
            fixed-order fp32 sums); called with std = 1 it adds 2 * 2^-24 |F_v| for a division the view kernel does not
            do: two units of slack per term, kept because the per-view bound is taken as that function returns it.
  unorient  the inverse of `views_ref.orient` moves values without arithmetic: an index image is sent through `orient`
            itself and every oriented pixel is put back where its index came from; a crop pixel that the kept canvas cut
            off receives nothing, the fill receives nothing.  Values and bounds move together.
  adds      n terms are added to a zero accumulator, view index ascending: (n + 1) 2^-24 sum_v |F_v| (n adds in any
            order, the first one exact), n = the views that reach the element.
  1 / std   fl(1 / std) and the product, once, after the sum: everything above divided by |std|, plus 2 * 2^-24 |ref|
            and the fp32 floor.  An element no view reaches has ref 0 and bound 2^-150: it must be exactly zero.
"""
import random

import torch
import torch.nn.functional as F

import preprocess_bwd_ref as pb
import views_ref as vr
from kernel_ref import EPS32, TINY, _f32c


def extent(view):
    """(oh, ow) of the oriented image of a plain-tuple view."""
    _, (x0, y0, x1, y1), turns, keep, _ = view
    w, h = x1 - x0, y1 - y0
    return (w, h) if turns % 2 == 1 and not keep else (h, w)


def unorient(T, h, w, turns, keep, flip, orient=vr.orient):
    """T (C, oh, ow) on the oriented image -> (C, h, w) on the crop, and the (h, w) mask of crop pixels that were reached."""
    index = torch.arange(1, h * w + 1).view(h, w)
    O = orient(index, turns, keep, flip)                 # which crop pixel each oriented pixel shows; 0: the fill
    live = O > 0
    out = torch.zeros(T.shape[0], h * w, dtype=T.dtype)
    out[:, O[live] - 1] = T[:, live]
    hit = torch.zeros(h * w, dtype=torch.bool)
    hit[O[live] - 1] = True
    return out.view(-1, h, w), hit.view(h, w)


def view_terms(G, views, S):
    """Per view: (src, box, unorient(F_v) (3, h, w) float64, its bound, the mask of crop pixels it reaches)."""
    out = []
    for v, view in enumerate(views):
        b, box, turns, keep, flip = vr.as_tuple(view)
        x0, y0, x1, y1 = box
        oh, ow = extent((b, box, turns, keep, flip))
        Fv, bv = pb.preprocess_bwd_ref(G[v:v + 1], oh, ow, S, 1.0, None, 1.0)
        Fc, hit = unorient(Fv[0], y1 - y0, x1 - x0, turns, keep, flip)
        bc, _ = unorient(bv[0], y1 - y0, x1 - x0, turns, keep, flip)
        out.append((b, box, Fc, bc, hit))
    return out


def views_bwd_ref(G, views, B, Hs, Ws, S, std, terms=None):
    """G fp32 (V, 3, S, S) -> (float64 ref (B, 3, Hs, Ws), per-element bound, n (B, Hs, Ws) views reaching each pixel)."""
    std = _f32c(std)
    acc = torch.zeros(B, 3, Hs, Ws, dtype=torch.float64)
    err, mag = torch.zeros_like(acc), torch.zeros_like(acc)
    n = torch.zeros(B, Hs, Ws, dtype=torch.float64)
    for b, (x0, y0, x1, y1), Fc, bc, hit in (view_terms(G, views, S) if terms is None else terms):
        acc[b, :, y0:y1, x0:x1] += Fc
        err[b, :, y0:y1, x0:x1] += bc
        mag[b, :, y0:y1, x0:x1] += Fc.abs()
        n[b, y0:y1, x0:x1] += hit
    ref = acc / std
    bound = (err + (n[:, None] + 1) * EPS32 * mag) / abs(std) + 2 * EPS32 * ref.abs() + TINY[torch.float32]
    return ref, bound, n


def torch_views(x, views, S, mean, std, orient=vr.orient):
    """crop -> `orient` -> F.interpolate(bilinear, antialias=True) -> (v - mean) / std per view by differentiable torch
    ops on the CPU in x's dtype: (V, 3, S, S), one graph over all views."""
    outs = []
    for view in views:
        b, (x0, y0, x1, y1), turns, keep, flip = vr.as_tuple(view)
        O = orient(x[b, :, y0:y1, x0:x1], turns, keep, flip)
        outs.append(F.interpolate(O[None], size=(S, S), mode="bilinear", antialias=True, align_corners=False))
    return (torch.cat(outs) - mean) / torch.tensor(_f32c(std), dtype=x.dtype)


def torch_autograd(G, views, B, Hs, Ws, S, std, dtype=torch.float64, orient=vr.orient):
    """torch's own autograd of `torch_views` in `dtype`: the gradient with respect to the sources for the output
    gradient G (the sources' values do not matter: linear)."""
    x = torch.zeros(B, 3, Hs, Ws, dtype=dtype, requires_grad=True)
    torch_views(x, views, S, 0.5, std, orient).backward(G.to(dtype))
    return x.grad


def grad_input(V, S, seed):
    return pb.grad_input(V, S, seed)


# ---- the view sets ---------------------------------------------------------------------------------------------------
# box (x0, y0, x1, y1): 51 x 34 (w - h odd), 50 x 34 (even), 37 x 37 (zero), 34 x 51 (odd, portrait); on 1 x 56 x 60, S = 42
ORIENT_BOXES = {"w-h_odd": (3, 5, 54, 39), "w-h_even": (4, 5, 54, 39), "square": (9, 2, 46, 39), "portrait_odd": (7, 1, 41, 52)}
ORIENT_KINDS = [(1, False, False), (2, False, False), (3, False, False), (1, True, False), (2, True, False),
                (3, True, False), (0, False, True), (1, False, True), (1, True, True), (3, True, True)]
ORIENT = [(0, box, t, k, f) for box in ORIENT_BOXES.values() for t, k, f in ORIENT_KINDS]

# name, box, S: on 2 x 240 x 235, each box as a view of image 1 then of image 0
SCALES = [
    ("upscale_8x8_box", (13, 21, 21, 29), 42),
    ("ratio16_33taps", (5, 9, 229, 233), 14),
    ("one_axis_identity_w42", (101, 3, 143, 100), 42),
    ("odd_offsets_nonint", (7, 11, 104, 142), 42),
    ("copy_shortcut_42x42", (31, 57, 73, 99), 42),
]
COPY_BOX = SCALES[4][1]

# image 0: nine overlapping views that all hold pixel (y 20, x 22) and leave a border; image 1: two; image 2: none
COVER_PIXEL = (20, 22)
COVERAGE = [
    (0, (4, 3, 40, 37), 0, False, False), (0, (10, 8, 30, 30), 1, False, False), (0, (12, 5, 33, 36), 2, False, False),
    (0, (8, 10, 38, 28), 3, False, False), (0, (15, 12, 29, 33), 1, True, False), (0, (6, 14, 36, 27), 3, True, False),
    (0, (18, 16, 28, 26), 0, False, True), (0, (5, 4, 39, 36), 1, False, True), (0, (16, 3, 30, 37), 2, True, True),
    (1, (2, 2, 20, 18), 0, False, False), (1, (25, 20, 43, 39), 1, True, False),
]


# 2 x 1040 x 1040: 2 x 65 x 65 = 8450 tiles of 16 x 16, above the 8192 blocks of the capped grid; GPU only (S = 80)
GRID_STRIDE = [
    (0, (0, 0, 1040, 1040), 0, False, False), (1, (0, 0, 1040, 1040), 1, True, False), (1, (5, 900, 1040, 1040), 3, False, True),
    (0, (1000, 3, 1040, 1037), 1, False, False), (1, (17, 1001, 97, 1040), 0, False, False),
]


def random_views(V, B, Hs, Ws, seed):
    """V valid records with a fixed seed: every source, turn, canvas rule and mirror, boxes from 3 pixels to the frame."""
    rng = random.Random(seed)
    out = []
    for n in range(V):
        w, h = rng.randint(3, Ws), rng.randint(3, Hs)
        x0, y0 = rng.randint(0, Ws - w), rng.randint(0, Hs - h)
        out.append((n % B if n < B else rng.randrange(B), (x0, y0, x0 + w, y0 + h), rng.randrange(4), rng.random() < 0.5,
                    rng.random() < 0.5))
    return out


def app_views(pp, h, w):
    """`detect_views(h, w).views` plus one exact three-quarter turn with a mirror and the mirrored frame, as plain tuples."""
    extra = [pp.View(0, (1, 2, w - 3, h - 1), turns=3, flip=True), pp.View(0, (0, 0, w, h), flip=True)]
    return [vr.as_tuple(v) for v in pp.detect_views(h, w).views + extra]


def cases(pp):
    """name -> (B, Hs, Ws, S, views): every call the tests make against the reference."""
    out = {"orientation": (1, 56, 60, 42, ORIENT)}
    for name, box, S in SCALES:
        out["scale_" + name] = (2, 240, 235, S, [(1, box, 0, False, False), (0, box, 0, False, False)])
    out["scale_copy_turn_and_flip"] = (2, 240, 235, 42, [(1, COPY_BOX, 1, False, False), (0, COPY_BOX, 0, False, True),
                                                        (0, COPY_BOX, 0, False, False)])
    out["coverage"] = (3, 40, 44, 12, COVERAGE)
    for V in (64, 65, 130):
        out[f"chunk_V{V}"] = (2, 50, 61, 45, random_views(V, 2, 50, 61, seed=1000 + V))
    out["app"] = (1, 70, 97, 42, app_views(pp, 70, 97))
    out["grid_stride"] = (2, 1040, 1040, 80, GRID_STRIDE)
    return out


CASE_NAMES = (["orientation"] + ["scale_" + s[0] for s in SCALES] + ["scale_copy_turn_and_flip", "coverage", "chunk_V64",
              "chunk_V65", "chunk_V130", "app"])
_cache = {}


def case_reference(pp, name, std=0.5):
    """(B, Hs, Ws, S, views, G, ref, bound, n) of a named case: computed once per process, shared, never modified."""
    key = (name, std)
    if key not in _cache:
        B, Hs, Ws, S, views = cases(pp)[name]
        G = grad_input(len(views), S, seed=sum(map(ord, name)))
        _cache[key] = (B, Hs, Ws, S, views, G) + views_bwd_ref(G, views, B, Hs, Ws, S, std)
    return _cache[key]
