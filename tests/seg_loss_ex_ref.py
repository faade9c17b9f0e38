"""float64 reference, element-wise bounds and an fp32 emulation for sgl_op_seg_loss_ex_fwd / _bwd (csrc/decoder_tail.hip):
`heads.combined_segmentation_loss` taken from the low-resolution logits.  A plain module: no tests.

z, p = sigmoid(z), bce and their error terms come from `kernel_ref.seg_pixels_ref` (the kernels form them as
sgl_op_seg_loss_fwd does).  Everything added here is derived from the fp32 operation count of the kernels' expressions, in
the style of kernel_ref (EPS32 = 2^-24 per rounding, DIV_ULPS for a division), never fitted to an output:

  q = (p + t) - 2 (p t)                 |1 - 2t| err(p) + 3 EPS32 (p + t + 2 p t)
  alpha_t = alpha t + (1-alpha)(1-t)    4 EPS32 alpha_t           (alpha is the float32 the kernel is handed)
  focal = alpha_t (q q) bce             alpha_t (2 q err(q) bce + q^2 err(bce)) + err(alpha_t) q^2 bce + 3 EPS32 focal
  boundary = (1 + 3 beta) bce           |1 + 3 beta| err(bce) + EPS32 |boundary|   (beta and 1 + 3 beta are exact integers)
  |p_a - p_b|                           err(p_a) + err(p_b) + EPS32 |p_a - p_b|; exactly 0, bound 0, where the two pixels have
                                        identical interpolation rows (clamped borders, g = 1)
  chunk sums                            as kernel_ref.seg_loss_fwd_ref: (8 ceil(S / 256) + BLOCK_TREE) EPS32 sum|terms|

  backward, per pixel (pq = p (1 - p): err(p) + 2 EPS32 pq;  d = p - t: err(p) + EPS32 |d|)
  F = (2 t D - 2 I) / D^2               kernel_ref.seg_loss_bwd_ref's (8 EPS32 + DIV_ULPS ulp)(|2 t D| + |2 I|) / D^2
  G = (t U - I (1-t)) / U^2             U = (P + T - I) + smooth rounds three times on terms of at most 3 U (I <= min(P, T)
                                        so U >= max(P, T)): 9 EPS32 relative, twice in U^2, once in t U; plus the products,
                                        the difference and the reciprocal: (26 EPS32 + DIV_ULPS ulp)(|t U| + |I (1-t)|) / U^2
  H = 2 q (1-2t) pq bce + q^2 d         2 |1-2t| (err(q) pq bce + q err(pq) bce + q pq err(bce)) + 2 q err(q) |d|
                                        + q^2 err(d) + 6 EPS32 (|first| + |second|)
  sign sum                              exact unless a pair is AMBIGUOUS: |p_a - p_b| in float64 <= err(p_a) + err(p_b), pairs
                                        with identical rows excepted.  Each ambiguous pair adds 2 |c_tv| pq to both its pixels.
  dz                                    the terms' errors + 6 EPS32 sum|terms|; gathered as kernel_ref.seg_loss_bwd_ref
"""
import math

import torch
import torch.nn.functional as F

import kernel_ref as kr
from kernel_ref import BLOCK_TREE, DIV_ULPS, EPS32, LOG2E, ULP32

FOCAL, BOUNDARY, TV = 1, 2, 4            # SGL_SEG_TERM_*
ALPHA = 0.25
MAX_AMBIGUOUS_SHARE = 0.002
# (B, g, S): what it exercises
CASES = [(2, 3, 42),      # S not a multiple of 8; last chunk of 2 rows; halo across chunks
         (2, 5, 37),      # odd S; idle threads
         (1, 1, 16),      # all taps coincide: TV exactly 0, boundary still live
         (1, 9, 7),       # S < g
         (1, 4, 260),     # S > 256: the strided column loop, and a TV pair across it
         (2, 27, 384)]    # the workload's ratio, once
MASK_KINDS = ["ones", "zeros", "rect_island", "noise"]


def mask_of(kind, S, gen_):
    """all ones; all zeros; a rectangle touching the top and left borders plus a one-pixel island; 0.3-density noise."""
    t = torch.zeros(S, S)
    if kind == "ones":
        t[:] = 1.0
    elif kind == "rect_island":
        t[: max(1, S // 2), : max(1, S // 3)] = 1.0
        t[S - 2, S - 2] = 1.0
    elif kind == "noise":
        t = (torch.rand(S, S, generator=gen_) < 0.3).float()
    return t


def inputs(B, g, S, mask_set, seed=None):
    """2.5 randn logits [B, g, g]; image b of mask set k carries MASK_KINDS[(k B + b) % 4]: the 4 // B sets of a case cover
    every kind.  coef [B, 6] in the magnitudes the wrapper produces (weight / N, weight / n, weight / pairs)."""
    gen_ = torch.Generator(device="cpu").manual_seed(seed if seed is not None else 1000 * g + S + 7 * mask_set)
    lr = torch.randn(B, g, g, generator=gen_) * 2.5
    tgt = torch.stack([mask_of(MASK_KINDS[(mask_set * B + b) % 4], S, gen_) for b in range(B)])
    N, pairs = float(B * S * S), float(B * S * (S - 1))
    coef = torch.tensor([[1.7 * 0.4 / N, -1.7 * 0.5 / B, 1.7 * 0.3 / N, 1.7 * 0.4 / N, -1.7 * 0.4 / B, 1.7 * 0.2 / pairs]]
                        ).repeat(B, 1)
    coef[1:] *= 0.5
    return lr, tgt, coef.float().contiguous()


def mask_sets(B):
    return range(4 // B)


def fold(partial):
    """The caller's fold of the chunks, in fp32 as the kernel reads it: [B, chunks, 8] -> [B, 8]."""
    return partial.double().sum(1).float().contiguous()


def _same_rows(W):
    """[S-1] bool: outputs k and k + 1 have the same interpolation row (W moves by g / S >= 1 / 2048 per output otherwise)."""
    return (W[1:] - W[:-1]).abs().amax(1) < 1e-9


def box_sum(t, pad_mode="zeros"):
    x = t[:, None]
    if pad_mode == "zeros":
        return F.conv2d(x, torch.ones(1, 1, 3, 3, dtype=t.dtype), padding=1)[:, 0]
    return F.conv2d(F.pad(x, (1, 1, 1, 1), mode="replicate"), torch.ones(1, 1, 3, 3, dtype=t.dtype))[:, 0]


def pixels(lr, tgt, alpha=ALPHA):
    """seg_pixels_ref plus the per-pixel terms of the enhanced loss with their bounds (module docstring), float64."""
    r = kr.seg_pixels_ref(lr, tgt)
    p, t, bce, ep, ebce = r["p"], r["t"], r["bce"], r["ep"], r["ebce"]
    a = kr._f32c(alpha)
    q = p + t - 2 * p * t
    eq = (1 - 2 * t).abs() * ep + 3 * EPS32 * (p + t + 2 * p * t)
    at = a * t + (1 - a) * (1 - t)
    eat = 4 * EPS32 * at
    focal = at * q * q * bce
    efocal = at * (2 * q * eq * bce + q * q * ebce) + eat * q * q * bce + 3 * EPS32 * focal.abs()
    s = box_sum(t)
    wb = 1 + 3 * ((s > 0).double() - (s == 9).double())
    bnd = wb * bce
    ebnd = wb.abs() * ebce + EPS32 * bnd.abs()
    same = _same_rows(r["W"])
    dx = p[:, :, 1:] - p[:, :, :-1]
    esx = ep[:, :, 1:] + ep[:, :, :-1]
    dy = p[:, 1:, :] - p[:, :-1, :]
    esy = ep[:, 1:, :] + ep[:, :-1, :]
    amb_x = (dx.abs() <= esx) & ~same[None, None, :]
    amb_y = (dy.abs() <= esy) & ~same[None, :, None]
    dx = torch.where(same[None, None, :], torch.zeros_like(dx), dx)
    dy = torch.where(same[None, :, None], torch.zeros_like(dy), dy)
    edx = torch.where(same[None, None, :], torch.zeros_like(dx), esx + EPS32 * dx.abs())
    edy = torch.where(same[None, :, None], torch.zeros_like(dy), esy + EPS32 * dy.abs())
    r.update(q=q, eq=eq, at=at, eat=eat, focal=focal, efocal=efocal, wb=wb, bnd=bnd, ebnd=ebnd, dx=dx, dy=dy, edx=edx,
             edy=edy, amb_x=amb_x, amb_y=amb_y, same=same)
    return r


def ambiguous_share(r):
    """(x, y): ambiguous pairs as a share of the pairs whose interpolation rows differ, per axis."""
    B, S = r["t"].shape[0], r["t"].shape[-1]
    live = max(1, int((~r["same"]).sum())) * S * B
    return int(r["amb_x"].sum()) / live, int(r["amb_y"].sum()) / live


def seg_loss_ex_fwd_ref(lr, tgt, alpha=ALPHA, terms=FOCAL | BOUNDARY | TV, r=None):
    """partial[b][chunk][8] = {sum bce, sum p t, sum p, sum t, sum focal, sum boundary, sum |dp/dx|, sum |dp/dy|} over 8
    output rows (the vertical pair (i, i + 1) in the chunk of row i), and its bound; unselected terms are exact zeros."""
    r = pixels(lr, tgt, alpha) if r is None else r
    B, S = tgt.shape[0], tgt.shape[-1]
    chunks = (S + 7) // 8
    depth = 8 * math.ceil(S / 256) + BLOCK_TREE
    z0 = torch.zeros(B, S, dtype=torch.float64)
    on = lambda bit, x: x if terms & bit else torch.zeros_like(x)
    rows = [r["bce"].sum(2), (r["p"] * r["t"]).sum(2), r["p"].sum(2), r["t"].sum(2), on(FOCAL, r["focal"].sum(2)),
            on(BOUNDARY, r["bnd"].sum(2)), on(TV, r["dx"].abs().sum(2)),
            on(TV, torch.cat([r["dy"].abs().sum(2), z0[:, :1]], 1))]
    mags = [r["bce"].abs().sum(2)] + rows[1:4] + [rows[4], on(BOUNDARY, r["bnd"].abs().sum(2))] + rows[6:]
    errs = [r["ebce"].sum(2), (r["t"] * r["ep"] + EPS32 * r["p"] * r["t"]).sum(2), r["ep"].sum(2), z0,
            on(FOCAL, r["efocal"].sum(2)), on(BOUNDARY, r["ebnd"].sum(2)), on(TV, r["edx"].sum(2)),
            on(TV, torch.cat([r["edy"].sum(2), z0[:, :1]], 1))]
    rows, mags, errs = torch.stack(rows, -1), torch.stack(mags, -1), torch.stack(errs, -1)        # [B, S, 8]
    ref = torch.zeros(B, chunks, 8, dtype=torch.float64)
    bound = torch.zeros(B, chunks, 8, dtype=torch.float64)
    for c in range(chunks):
        sl = slice(8 * c, min(8 * c + 8, S))
        ref[:, c] = rows[:, sl].sum(1)
        bound[:, c] = errs[:, sl].sum(1) + depth * EPS32 * mags[:, sl].sum(1)
    return ref, bound


def _neighbour_sum(dx, dy, fn):
    """Per pixel, sum over its <= 4 pairs of fn(own - neighbour) given dx = p[j+1] - p[j], dy = p[i+1] - p[i]."""
    B, S = dx.shape[0], dx.shape[1]
    out = torch.zeros(B, S, S, dtype=torch.float64)
    out[:, :, :-1] += fn(-dx)
    out[:, :, 1:] += fn(dx)
    out[:, :-1, :] += fn(-dy)
    out[:, 1:, :] += fn(dy)
    return out


def pixel_grad_ref(r, sums, coef, terms, eps, smooth):
    """dz per output pixel and its bound (module docstring) from the fp32 sums / coef the kernel reads."""
    p, t, ep = r["p"], r["t"], r["ep"]
    s64, c64 = sums.double(), coef.double().clone()
    for k, bit in ((2, FOCAL), (3, BOUNDARY), (5, TV)):
        if not terms & bit:
            c64[:, k] = 0
    c = [c64[:, k, None, None] for k in range(6)]
    I, Ps, Ts = (s64[:, k, None, None] for k in (1, 2, 3))
    D = Ps + Ts + kr._f32c(eps)
    U = Ps + Ts - I + kr._f32c(smooth)
    Fd = (2 * t * D - 2 * I) / (D * D)
    eFd = (8 * EPS32 + DIV_ULPS * ULP32) * ((2 * t * D).abs() + (2 * I).abs()) / (D * D)
    G = (t * U - I * (1 - t)) / (U * U)
    eG = (26 * EPS32 + DIV_ULPS * ULP32) * ((t * U).abs() + (I * (1 - t)).abs()) / (U * U)
    pq, d = p * (1 - p), p - t
    epq, ed = ep + 2 * EPS32 * pq, ep + EPS32 * (p - t).abs()
    q, eq, at, eat, bce, ebce = r["q"], r["eq"], r["at"], r["eat"], r["bce"], r["ebce"]
    h1, h2 = 2 * q * (1 - 2 * t) * pq * bce, q * q * d
    H = h1 + h2
    eH = 2 * (1 - 2 * t).abs() * (eq * pq * bce + q * epq * bce + q * pq * ebce) + 2 * q * eq * d.abs() + q * q * ed + \
        6 * EPS32 * (h1.abs() + h2.abs())
    sg = _neighbour_sum(r["dx"], r["dy"], torch.sign)
    namb = _neighbour_sum(r["amb_x"].double(), r["amb_y"].double(), torch.abs)
    tm = [c[0] * d, c[1] * pq * Fd, c[2] * at * H, c[3] * r["wb"] * d, c[4] * pq * G, c[5] * pq * sg]
    te = [c[0].abs() * ed + EPS32 * tm[0].abs(),
          c[1].abs() * (ep * Fd.abs() + pq * (eFd + 4 * EPS32 * Fd.abs())),
          c[2].abs() * (eat * H.abs() + at * eH + 2 * EPS32 * at * H.abs()),
          c[3].abs() * r["wb"].abs() * ed + 2 * EPS32 * tm[3].abs(),
          c[4].abs() * (ep * G.abs() + pq * (eG + 4 * EPS32 * G.abs())),
          c[5].abs() * (sg.abs() * epq + 2 * pq * namb) + 2 * EPS32 * tm[5].abs()]
    dz = sum(tm)
    edz = sum(te) + 6 * EPS32 * sum(x.abs() for x in tm)
    return dz, edz


def seg_loss_ex_bwd_ref(lr, tgt, sums, coef, alpha=ALPHA, terms=FOCAL | BOUNDARY | TV, eps=1e-6, smooth=1e-6, r=None):
    """dlogits_lr = W^T dz W and its bound; the gather's own error as kernel_ref.seg_loss_bwd_ref (position error of the
    weights on either axis, the accumulation over the rows and columns that feed one low-res pixel)."""
    r = pixels(lr, tgt, alpha) if r is None else r
    W, Dm = r["W"], r["Dm"].abs()
    dz, edz = pixel_grad_ref(r, sums, coef, terms, eps, smooth)
    ref = W.t() @ dz @ W
    cnt = (W > 0).sum(0).double()
    adz = W.t() @ dz.abs() @ W
    bound = W.t() @ edz @ W + r["cs"] * (Dm.t() @ dz.abs() @ W + W.t() @ dz.abs() @ Dm) + \
        (cnt[:, None] + cnt[None, :] + 8) * EPS32 * adz + EPS32 * ref.abs()
    return ref, bound


# ---- fp32 emulation ---------------------------------------------------------------------------------------------
MUTANTS = ("beta_nopad", "tvy_wrong_chunk", "iou_tU_minus_I", "focal_no_dq")


def emulate(lr, tgt, sums, coef, alpha=ALPHA, terms=FOCAL | BOUNDARY | TV, eps=1e-6, smooth=1e-6, mutant=None):
    """Both kernels' per-pixel arithmetic in torch fp32 (taps, lerps and expressions as the kernels order them, the weight
    0 where the two taps of an axis coincide); sums and the gather by plain fp32 torch reductions.
    Returns partial [B, chunks, 8], dlogits_lr [B, g, g].  Mutants (the host test asserts each leaves the bounds):
      beta_nopad       beta from a 3x3 box with replicated instead of zero padding
      tvy_wrong_chunk  the vertical pair (i, i + 1) summed into the chunk of row i + 1
      iou_tU_minus_I   the IoU derivative with t U - I in place of t U - I (1 - t)
      focal_no_dq      the focal derivative without its dq/dz term"""
    assert mutant is None or mutant in MUTANTS
    B, g, S = lr.shape[0], lr.shape[-1], tgt.shape[-1]
    f = torch.float32
    c = lambda v: torch.tensor(v, dtype=f)
    scale = c(float(g)) / c(float(S))
    i = torch.arange(S, dtype=f)
    s = (scale * (i + 0.5) - 0.5).clamp_min(0.0)
    i0 = s.floor().clamp_max(g - 1).long()
    i1 = (i0 + 1).clamp_max(g - 1)
    w = torch.where(i0 == i1, torch.zeros_like(s), s - i0.to(f))
    L, t = lr.float(), tgt.float()
    wx, wy = w[None, None, :], w[None, :, None]
    top = L[:, i0][:, :, i0] * (1 - wx) + L[:, i0][:, :, i1] * wx
    bot = L[:, i1][:, :, i0] * (1 - wx) + L[:, i1][:, :, i1] * wx
    z = top * (1 - wy) + bot * wy
    e = torch.exp2(-z.abs() * c(LOG2E))
    bce = z.clamp_min(0) - z * t + torch.log1p(e)
    p = torch.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    a = c(alpha)
    q = (p + t) - 2.0 * (p * t)
    at = a * t + (1 - a) * (1 - t)
    sbox = box_sum(t, "replicate" if mutant == "beta_nopad" else "zeros")
    wb = 1 + 3 * ((sbox > 0).to(f) - (sbox == 9).to(f))
    dx = (p[:, :, 1:] - p[:, :, :-1])
    dy = (p[:, 1:, :] - p[:, :-1, :])
    z1 = torch.zeros(B, 1, dtype=f)
    tvy_rows = torch.cat([z1, dy.abs().sum(2)], 1) if mutant == "tvy_wrong_chunk" else torch.cat([dy.abs().sum(2), z1], 1)
    on = lambda bit, x: x if terms & bit else torch.zeros_like(x)
    rows = torch.stack([bce.sum(2), (p * t).sum(2), p.sum(2), t.sum(2), on(FOCAL, (at * (q * q) * bce).sum(2)),
                        on(BOUNDARY, (wb * bce).sum(2)), on(TV, dx.abs().sum(2)), on(TV, tvy_rows)], -1)
    chunks = (S + 7) // 8
    part = torch.stack([rows[:, 8 * k:8 * k + 8].sum(1) for k in range(chunks)], 1)

    cf, sm = coef.float(), sums.float()
    k_ = [cf[:, k, None, None] for k in range(6)]
    I, Ps, Ts = (sm[:, k, None, None] for k in (1, 2, 3))
    D = Ps + Ts + c(eps)
    U = (Ps + Ts - I) + c(smooth)
    invD2, invU2 = 1.0 / (D * D), 1.0 / (U * U)
    pq, d = p * (1 - p), p - t
    dz = k_[0] * d + k_[1] * pq * ((2 * t * D - 2 * I) * invD2)
    iou_num = (t * U - I) if mutant == "iou_tU_minus_I" else (t * U - I * (1 - t))
    dz = dz + k_[4] * pq * (iou_num * invU2)
    if terms & FOCAL:
        first = torch.zeros_like(p) if mutant == "focal_no_dq" else 2 * q * (1 - 2 * t) * pq * bce
        dz = dz + k_[2] * at * (first + q * q * d)
    if terms & BOUNDARY:
        dz = dz + k_[3] * wb * d
    if terms & TV:
        dz = dz + k_[5] * pq * _neighbour_sum(dx.double(), dy.double(), torch.sign).to(f)
    Wm = torch.zeros(S, g, dtype=f)
    r_ = torch.arange(S)
    Wm[r_, i0] += 1 - w
    Wm[r_, i1] += w
    return part, Wm.t() @ dz @ Wm
