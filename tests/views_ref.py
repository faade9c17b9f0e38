"""float64 reference and per-element bound for sgl_op_preprocess_views (csrc/preprocess.hip): the app's test-time views.

By the conventions at the top of tests/kernel_ref.py.  A view is crop -> orient -> resize -> normalise -> layout.  Crop and
orientation move source values (or the exact fill 0) without arithmetic, so the reference builds the oriented image in
the SOURCE's own dtype and hands it to `kernel_ref.resize_ref`, `normalise_ref` and `patch_major`, imported and
unmodified: the bound of a view is the bound of sgl_op_preprocess on its oriented image, nothing added.

`keep_canvas` restates what PIL's `Image.rotate(90 k)` returns with its defaults (expand=False, nearest, fill 0) as the
integer rule of include/siglip_hip.h; tests/test_views_host.py pins it to PIL itself.  PIL's nearest affine transform
samples input pixel floor(a (x + 0.5) + b (y + 0.5) + c) of output pixel (x, y); for a quarter turn about the centre
(w / 2, h / 2) that is

    one turn     column floor((w + h) / 2 - (y + 0.5)) = ((w + h - 1) >> 1) - y,   row ((h - w + 1) >> 1) + x
    three turns  column ((w - h + 1) >> 1) + y,                                    row ((w + h - 1) >> 1) - x

(>> floors, for the negative half-integers too); two turns is the exact rotation (PIL transposes).
"""
import torch

import kernel_ref as kr


def keep_canvas_index(h, w, turns):
    """(row, column, inside) of the crop pixel that lands on each pixel of the kept h x w canvas."""
    y, x = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    if turns == 1:
        cx, cy = ((w + h - 1) >> 1) - y, ((h - w + 1) >> 1) + x
    elif turns == 2:
        cx, cy = w - 1 - x, h - 1 - y
    else:
        cx, cy = ((w - h + 1) >> 1) + y, ((w + h - 1) >> 1) - x
    inside = (cx >= 0) & (cx < w) & (cy >= 0) & (cy < h)
    return cy.clamp(0, h - 1), cx.clamp(0, w - 1), inside


def orient(C, turns, keep_canvas, flip):
    """C (..., h, w) of any dtype -> the oriented image O: values moved, fill 0, nothing computed."""
    h, w = C.shape[-2:]
    if turns == 0:
        O = C
    elif not keep_canvas:
        O = torch.rot90(C, turns, dims=(-2, -1))           # counter-clockwise, numpy.rot90's convention
    else:
        cy, cx, inside = keep_canvas_index(h, w, turns)
        O = torch.where(inside, C[..., cy, cx], torch.zeros((), dtype=C.dtype))
    return O.flip(-1) if flip else O


def oriented_source(src, src_u8, view):
    """The oriented image of one view in the layout `kernel_ref.resize_ref` reads: uint8 (1, oh, ow, 3) or float32
    (1, 3, oh, ow).  `view`: (src, (x0, y0, x1, y1), turns, keep_canvas, flip)."""
    b, (x0, y0, x1, y1), turns, keep, flip = view
    img = src[b].permute(2, 0, 1) if src_u8 else src[b]                        # (3, Hs, Ws)
    O = orient(img[:, y0:y1, x0:x1], turns, keep, flip).contiguous()
    return O.permute(1, 2, 0)[None].contiguous() if src_u8 else O[None]


def as_tuple(v):
    """A siglip_amd.preprocess.View (or a tuple already) -> the plain tuple this module reads."""
    return v if isinstance(v, tuple) else (v.src, tuple(v.box), v.turns, bool(v.keep_canvas), bool(v.flip))


def views_resized_ref(src, src_u8, views, S):
    """float64 (V, 3, S, S) in [0, 1] before normalisation, and its bound."""
    outs, bounds = zip(*(kr.resize_ref(oriented_source(src, src_u8, as_tuple(v)), src_u8, S) for v in views))
    return torch.cat(outs), torch.cat(bounds)


def views_ref(src, src_u8, views, S, P, Kp, patch, mean, std, out_dt):
    """The reference of sgl_op_preprocess_views and its per-element bound, (V, 3, S, S) or [V g g, Kp]."""
    v, ev = views_resized_ref(src, src_u8, views, S)
    out, bound = kr.normalise_ref(v, ev, mean, std, out_dt)
    return kr.patch_major(out, bound, P, Kp) if patch else (out, bound)
