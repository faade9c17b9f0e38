"""Reference for sgl_op_preprocess_aug_bwd (csrc/preprocess.hip), the adjoint of the augmenting input transform
resize -> flip -> rotation -> colour jitter -> normalise with respect to its source.

`forward` restates `oracle.preprocess_oracle.augment_transform` operator by operator in a dtype of the caller's choice
(float64: the reference; float32: the yardstick of what fp32 arithmetic costs), with the explicit separable resize of
`triangle_resize` (the oracle's fp32 weights as two matrices).  The gradient comes from torch.autograd, whose conventions
where the transform is not differentiable are the contract of the kernel (tests/test_aug_bwd_host.py pins them).

Next to the output, `forward` returns per output pixel the flag "within DELTA of a kink": a clamp's argument against 0 or 1,
a pairwise difference of the three channels entering the hue step against 0, or 6 h (h the shifted hue) against an
integer differs from its kink by more than 0 and less than DELTA.  Exact equality is not flagged: the conventions decide
it.  The colour tests zero the cotangent on flagged pixels; the vector-Jacobian product is linear in the cotangent and
every colour term is per-pixel multiplicative in it, so such a pixel cannot influence any element of d_src and every
element is compared.  At most KINK_SHARE of a case's pixels may be flagged.

Geometry alone (no colour operators) is linear: `geometry_ref` is the float64 adjoint with a per-element bound derived
from the kernel's operations, on top of tests/preprocess_bwd_ref.py.
"""
import itertools
import math

import torch

import kernel_ref as kr
import preprocess_bwd_ref as pb
from kernel_ref import EPS32, _f32c

DELTA = 1e-4
KINK_SHARE = 0.03
FLOOR = 32 * EPS32               # of max|ref| and of |ref|_2: the floor of the colour bound
MARGIN = 8.0                     # kernel error <= MARGIN x the error of the fp32 restatement, per metric
W_GREY = (0.299, 0.587, 0.114)
PARAM_SETS = [(1.3, 1.4, 1.5, 0.2), (0.7, 0.6, 0.5, -0.3), (1.1, 0.9, 1.1, 0.05)]    # brightness, contrast, saturation, hue
ORDERS = [list(p) for p in itertools.permutations(range(4))]


def _oracle():
    import __graft_entry__ as g
    g.load_oracle()                                        # puts nothing on sys.path: import the sibling by file
    import importlib.util
    import os
    import sys
    name = "preprocess_oracle"
    if name not in sys.modules:
        spec = importlib.util.spec_from_file_location(name, os.path.join(g.ROOT, "oracle", "preprocess_oracle.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
    return sys.modules[name]


def record(flip=False, angle=0.0, factors=(1.0, 1.0, 1.0, 0.0), order=None):
    """One per-sample dict in the format of preprocess.sample_augmentation, floats rounded to fp32 (what the device table
    holds), so that the reference and the kernel read the same numbers."""
    a = math.radians(angle)
    b, c, s, h = (_f32c(v) for v in factors)
    return dict(flip=bool(flip), cos=_f32c(math.cos(a)) if a else 1.0, sin=_f32c(math.sin(a)) if a else 0.0,
                brightness=b, contrast=c, saturation=s, hue=h, order=list(order) if order is not None else None)


def _resize_matrix(S, n_in, dtype, device="cpu"):
    W = torch.zeros(S, n_in, dtype=dtype)
    for o, (lo, w) in enumerate(_oracle().aa_weights(S, n_in)):
        W[o, lo:lo + len(w)] = torch.from_numpy(w).to(dtype)
    return W.to(device)


def _near(v, kink):
    d = (v - kink).abs()
    return (d > 0) & (d < DELTA)


def _clamp(u, flag):
    """clamp(u, 0, 1) on (3, S, S); flags the pixels with a channel near either bound."""
    with torch.no_grad():
        flag |= (_near(u, 0.0) | _near(u, 1.0)).any(0)
    return u.clamp(0, 1)


def _grey(x):
    return W_GREY[0] * x[0:1] + W_GREY[1] * x[1:2] + W_GREY[2] * x[2:3]


def _hue(x, shift, flag):
    """`_rgb2hsv` -> (h + shift) % 1 -> `_hsv2rgb` of the oracle on (3, S, S), line by line."""
    r, g, b = x.unbind(0)
    with torch.no_grad():
        flag |= _near(r - g, 0.0) | _near(r - b, 0.0) | _near(g - b, 0.0)
    maxc = torch.max(x, dim=0).values
    minc = torch.min(x, dim=0).values
    eqc = maxc == minc
    cr = maxc - minc
    ones = torch.ones_like(maxc)
    s = cr / torch.where(eqc, ones, maxc)
    cr_divisor = torch.where(eqc, ones, cr)
    rc, gc, bc = (maxc - r) / cr_divisor, (maxc - g) / cr_divisor, (maxc - b) / cr_divisor
    hr = (maxc == r) * (bc - gc)
    hg = ((maxc == g) & (maxc != r)) * (2.0 + rc - bc)
    hb = ((maxc != g) & (maxc != r)) * (4.0 + gc - rc)
    h = torch.fmod((hr + hg + hb) / 6.0 + 1.0, 1.0)
    h = (h + shift) % 1.0
    v = maxc
    h6 = h * 6.0
    with torch.no_grad():
        flag |= _near(h6, h6.round())
    i = torch.floor(h6)
    f = h6 - i
    i = i.to(torch.int32) % 6
    pqt = _clamp(torch.stack((v * (1.0 - s), v * (1.0 - f * s), v * (1.0 - (1.0 - f) * s))), flag)
    p, q, t = pqt.unbind(0)
    mask = i.unsqueeze(0) == torch.arange(6, device=x.device).view(-1, 1, 1)
    a1 = torch.stack((v, q, p, p, t, v))
    a2 = torch.stack((t, v, v, q, p, p))
    a3 = torch.stack((p, p, t, v, v, q))
    a4 = torch.stack((a1, a2, a3))
    return torch.einsum("ijk, xijk -> xjk", mask.to(dtype=x.dtype), a4)


def _rotate(x, cos_a, sin_a):
    """`rotate_bilinear_zeros` of the oracle in x's dtype."""
    S = x.shape[-1]
    ctr = 0.5 * (S - 1)
    ar = torch.arange(S, dtype=x.dtype, device=x.device)
    ys, xs = torch.meshgrid(ar, ar, indexing="ij")
    dx, dy = xs - ctr, ys - ctr
    sx = cos_a * dx - sin_a * dy + ctr
    sy = sin_a * dx + cos_a * dy + ctr
    x0, y0 = torch.floor(sx), torch.floor(sy)
    fx, fy = sx - x0, sy - y0
    out = torch.zeros_like(x)
    for jy in (0, 1):
        for jx in (0, 1):
            yy, xx = (y0 + jy).long(), (x0 + jx).long()
            w = (fy if jy else 1.0 - fy) * (fx if jx else 1.0 - fx)
            ok = (yy >= 0) & (yy < S) & (xx >= 0) & (xx < S)
            out = out + torch.where(ok, w, torch.zeros_like(w)) * x[:, yy.clamp(0, S - 1), xx.clamp(0, S - 1)]
    return out


def forward(x, size, params, mean=0.5, std=0.5):
    """x (B, 3, Hs, Ws) in float64 or float32 (uint8 NHWC sources: pass bytes / 255 as NCHW) -> (out (B, 3, S, S) in x's
    dtype, flagged (B, S, S) bool).  Differentiable with respect to x; runs on x's device (tests/bench_aug_grad.py times
    it there as the per-operator torch route)."""
    B, _, Hs, Ws = x.shape
    if (Hs, Ws) != (size, size):
        x = _resize_matrix(size, Hs, x.dtype, x.device) @ x @ _resize_matrix(size, Ws, x.dtype, x.device).t()
    outs, flags = [], []
    for b, pr in enumerate(params):
        im = x[b]
        flag = torch.zeros(size, size, dtype=torch.bool, device=x.device)
        if pr["flip"]:
            im = im.flip(-1)
        if not (pr["cos"] == 1.0 and pr["sin"] == 0.0):
            im = _rotate(im, pr["cos"], pr["sin"])
        for op in (pr["order"] or []):
            if op == 0:
                im = _clamp(im * pr["brightness"], flag)
            elif op == 1:
                m = _grey(im).mean()
                im = _clamp((im - m) * pr["contrast"] + m, flag)
            elif op == 2:
                g = _grey(im)
                im = _clamp((im - g) * pr["saturation"] + g, flag)
            else:
                im = _hue(im, pr["hue"], flag)
        outs.append(im)
        flags.append(flag)
    return (torch.stack(outs) - mean) / std, torch.stack(flags)


def as_float(src, dtype):
    """A source batch (uint8 NHWC or float NCHW) as the (B, 3, Hs, Ws) tensor the gradient is taken with respect to."""
    if src.dtype == torch.uint8:
        return src.permute(0, 3, 1, 2).to(dtype) / 255.0
    return src.to(dtype)


def vjp(src, size, params, cot, std=0.5, dtype=torch.float64):
    """d_src (B, 3, Hs, Ws) in `dtype` by torch.autograd for the cotangent `cot` (B, 3, S, S)."""
    x = as_float(src, dtype).clone().requires_grad_(True)
    out, _ = forward(x, size, params, 0.5, std)
    out.backward(cot.to(dtype))
    return x.grad


def flags_of(src, size, params):
    with torch.no_grad():
        return forward(as_float(src, torch.float64), size, params)[1]


def masked_cotangent(src, size, params, seed):
    """(cot fp32 (B, 3, S, S), unit variance and zero on the flagged pixels; the flagged share per image)."""
    flag = flags_of(src, size, params)
    B = flag.shape[0]
    cot = pb.grad_input(B, size, seed) * (~flag)[:, None]
    return cot, flag.flatten(1).double().mean(1)


def metrics(got, ref):
    """(max|e| / max|ref|, |e|_2 / |ref|_2) per image."""
    e = (got.double() - ref).flatten(1)
    r = ref.flatten(1)
    return e.abs().amax(1) / r.abs().amax(1), e.norm(dim=1) / r.norm(dim=1)


def colour_bound(src, size, params, cot, ref, std=0.5):
    """Per image and metric: MARGIN x the error of the fp32 restatement under autograd against the float64 one, at least
    MARGIN x ... is never below FLOOR."""
    m_inf, m_l2 = metrics(vjp(src, size, params, cot, std, torch.float32), ref)
    return (MARGIN * m_inf).clamp_min(FLOOR), (MARGIN * m_l2).clamp_min(FLOOR)


# ---- the cases tests/test_aug_bwd_gpu.py runs and tests/test_aug_bwd_host.py checks the kink share of -------------------
def uniform_source(B, Hs, Ws, u8, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    if u8:
        return torch.randint(0, 256, (B, Hs, Ws, 3), generator=g, dtype=torch.uint8)
    return torch.rand(B, 3, Hs, Ws, generator=g)


def colour_case(n):
    """Parameter set n at Hs = Ws = S = 16: the 24 orders (contrast with zero to three operators in front of it, six
    times each), then each operator alone: its factor, the others neutral (1, 1, 1, 0).  The lone operator stands at the
    END of its order: a neutral contrast, saturation or hue step is the identity only up to rounding, so behind a clamp
    that saturated a channel its argument sits 1e-16 off the bound, which the flag rule counts as a kink (6 % of the
    pixels with brightness 1.3 in front), while in front of it it sees the unsaturated source.  (source, S, records)."""
    fac = PARAM_SETS[n]
    recs = [record(factors=fac, order=o) for o in ORDERS]
    neutral = (1.0, 1.0, 1.0, 0.0)
    for op in range(4):
        alone = tuple(fac[k] if k == op else neutral[k] for k in range(4))
        recs.append(record(factors=alone, order=[k for k in range(4) if k != op] + [op]))
    return uniform_source(len(recs), 16, 16, False, seed=100 + n), 16, recs


def everything_case(u8):
    """30 x 37 -> 24, three images: flips, angles and orders differ; one record without colour operators."""
    recs = [record(True, 5.0, PARAM_SETS[0], [1, 3, 0, 2]), record(False, -30.0, PARAM_SETS[1], None),
            record(True, 0.0, PARAM_SETS[2], [3, 2, 1, 0])]
    return uniform_source(3, 30, 37, u8, seed=110 + int(u8)), 24, recs


GEOMETRY_RECORDS = [record(True), record(True, 5.0), record(False, -30.0)]
GEOMETRIES = [((30, 37), 24), ((11, 13), 16), ((24, 24), 24)]
# B 3 Hs Ws > 2048 x 256, the capped grid of the resize adjoint (the other kernels launch one block per 256 pixels)
GRID_CASE = ((300, 300), 24, 2)


# ---- geometry alone: float64 adjoint and derived bound -------------------------------------------------------------------
def _rotation_matrix(S, cos_a, sin_a):
    """R [S S, S S] float64 with T = R F on flattened images, E the per-weight error bound on the taps the fp32 kernel can
    have, n the number of outputs an intermediate pixel can receive from.  The fp32 sample position is off by at most
    4 * 2^-24 S per axis (two products of magnitude <= S / 2, two sums of magnitude <= S: the count of
    kernel_ref.aug_ref); a bilinear weight moves by at most the sum of both, and a tap the fp32 floor gains or loses has
    a weight below it: (8 S + 8) 2^-24 on every tap within 1 + that of the sample point; 3 more roundings for
    1 - f, the product and the multiply with g."""
    ctr = 0.5 * (S - 1)
    ar = torch.arange(S, dtype=torch.float64)
    ys, xs = torch.meshgrid(ar, ar, indexing="ij")
    dx, dy = xs - ctr, ys - ctr
    sx = (cos_a * dx - sin_a * dy + ctr).flatten()
    sy = (sin_a * dx + cos_a * dy + ctr).flatten()
    ux, uy = xs.flatten()[None, :], ys.flatten()[None, :]
    wx = (1.0 - (sx[:, None] - ux).abs()).clamp_min(0.0)
    wy = (1.0 - (sy[:, None] - uy).abs()).clamp_min(0.0)
    R = wy * wx
    dpos = (8 * S + 8) * EPS32
    reach = ((sx[:, None] - ux).abs() < 1.0 + dpos) & ((sy[:, None] - uy).abs() < 1.0 + dpos)
    E = dpos * reach + 3 * EPS32 * R
    return R, E, reach.sum(0).double()


def geometry_ref(G, Hs, Ws, S, std, params):
    """G fp32 (B, 3, S, S), records without colour operators -> (float64 d_src (B, 3, Hs, Ws), per-element bound):
    d_R = flip^T R^T G with the bound E^T |G| + (n + 1) 2^-24 (R + E)^T |G| of the gather's sum, then the resize adjoint
    of preprocess_bwd_ref on d_R, whose own bound takes d_R as exact, plus d_R's error through the widened |weights|."""
    G64 = G.double()
    B = G.shape[0]
    dR, eR = torch.zeros_like(G64), torch.zeros_like(G64)
    for b, pr in enumerate(params):
        assert pr["order"] is None
        g, e = G64[b], torch.zeros_like(G64[b])
        if not (pr["cos"] == 1.0 and pr["sin"] == 0.0):
            R, E, n = _rotation_matrix(S, pr["cos"], pr["sin"])
            gf, af = g.flatten(1), g.abs().flatten(1)
            e = (af @ E + (n + 1) * EPS32 * (af @ (R + E))).view(3, S, S)
            g = (gf @ R).view(3, S, S)
        if pr["flip"]:
            g, e = g.flip(-1), e.flip(-1)
        dR[b], eR[b] = g, e
    ref, bound = pb.preprocess_bwd_ref(dR, Hs, Ws, S, std, None, 1.0)
    if Hs == S and Ws == S:
        through = eR
    else:
        Wy, Ey, _ = pb._axis(S, Hs)
        Wx, Ex, _ = pb._axis(S, Ws)
        through = (Wy + Ey).t() @ eR @ (Wx + Ex)
    return ref, bound + through / abs(_f32c(std)) * (1 + 4 * EPS32)
