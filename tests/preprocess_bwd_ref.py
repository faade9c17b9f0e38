"""float64 reference, per-element bound and fp32 emulation for sgl_op_preprocess_bwd, the adjoint of
Resize(S, antialias=True) -> [MixUp] -> Normalize with respect to a float source (csrc/preprocess.hip).

Built on `kernel_ref.aa_axis`, by the conventions at the top of tests/kernel_ref.py: the reference is the same operation in
float64 on the fp32 gradient the kernel received, the bound is per element and derived, not fitted:

    F[j]     = Wy^T G[j] Wx                                   one image's filter sum, (Hs, S) (S, S) (S, Ws)
    d_src[b] = (lam F[b] + (1 - lam) sum_{j : mix[j] = b} F[j]) / std

  weights   `aa_axis` bounds sum_j |w_fp32 - w| of one OUTPUT by A[o]; the adjoint reads single weights of many outputs, so
            every weight of output o carries A[o] whole: E[o, j] = A[o] on the taps the fp32 filter can have.  Those are the
            float64 taps with a positive weight widened by one tap on either side: the float64 range [lo, hi) holds at
            most one zero-weight tap (hi - 1, when centre + support + 0.5 is an integer), and the fp32 range differs from
            it by at most one tap at either end (both ends are truncations of values 2^-24-close to the float64 ones).
            |wy wx - Wy Wx| <= |Wy| Ex + Ey |Wx| + Ey Ex, summed against |G|.
  sums      the kernel's order is fixed: a row sum of cx products, then cy products and adds, cy / cx the number of
            outputs that cover the source row / column (counted on the widened taps): (cy + cx + 2) 2^-24 sum|terms|.
  MixUp     lam F[b] + fl(1 - lam) F[j] + ...: the rounding of 1 - lam, one product and one add per term as
            `preprocess_ref` counts them (3 * 2^-24 for the forward's two terms); image b is referenced by r[b] images, so
            a term passes r[b] adds: (2 + r[b]) 2^-24 sum|terms| (r = 1, the forward's case, gives the 3).
  1 / std   fl(1 / std) and the product: 2 * 2^-24 |ref|, everything above divided by |std|.
  Hs == S and Ws == S is the kernel's copy shortcut: F[j] = G[j] exactly.
"""
import torch
import torch.nn.functional as F

import kernel_ref as kr
from kernel_ref import EPS32, TINY, _f32c

# (Hs, Ws) -> S of the issue's CPU check against torch's own float64 autograd
GEOMETRIES = [((97, 131), 42), ((30, 30), 42), ((42, 97), 42), ((224, 224), 14), ((50, 50), 45), ((7, 9), 112)]
MIXES = [(None, 1.0), ([1, 1, 0], 0.0), ([1, 1, 0], 0.3), ([1, 1, 0], 1.0)]


def grad_input(B, S, seed):
    """Unit-variance fp32 `d loss / d out` (B, 3, S, S) on the CPU."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(B, 3, S, S, generator=g)


def _axis(S, n_in):
    """W [S, in] float64, E [S, in] the per-weight error on the taps the fp32 filter can have."""
    W, A = kr.aa_axis(S, n_in)
    live = (W > 0).double()
    wide = live.clone()
    wide[:, 1:] = torch.maximum(wide[:, 1:], live[:, :-1])
    wide[:, :-1] = torch.maximum(wide[:, :-1], live[:, 1:])
    return W, A[:, None] * wide, wide.sum(0)


def preprocess_bwd_ref(G, Hs, Ws, S, std, mix_index, lam):
    """G fp32 (B, 3, S, S) -> (float64 ref (B, 3, Hs, Ws), per-element bound)."""
    G64 = G.double()
    B = G.shape[0]
    std = _f32c(std)
    if Hs == S and Ws == S:
        Fs, eF = G64, torch.zeros_like(G64)
    else:
        Wy, Ey, cy = _axis(S, Hs)
        Wx, Ex, cx = _axis(S, Ws)
        aG = G64.abs()
        Fs = Wy.t() @ G64 @ Wx
        mag = (Wy + Ey).t() @ aG @ (Wx + Ex)
        werr = Wy.t() @ aG @ Ex + Ey.t() @ aG @ Wx + Ey.t() @ aG @ Ex
        eF = werr + (cy[:, None] + cx[None, :] + 2) * EPS32 * mag
    if mix_index is None:
        v, ev = Fs, eF
    else:
        lam = _f32c(lam)
        idx = torch.as_tensor(mix_index).long()
        v, ev, mag = lam * Fs, abs(lam) * eF, (lam * Fs).abs()
        refs = torch.zeros(B, dtype=torch.float64)
        tail, etail, mtail = torch.zeros_like(Fs), torch.zeros_like(Fs), torch.zeros_like(Fs)
        for j in range(B):
            b = int(idx[j])
            t = (1.0 - lam) * Fs[j]
            tail[b] += t
            etail[b] += abs(1.0 - lam) * eF[j]
            mtail[b] += t.abs()
            refs[b] += 1
        v = v + tail
        ev = ev + etail + (2 + refs)[:, None, None, None] * EPS32 * (mag + mtail)
    ref = v / std
    return ref, ev / abs(std) + 2 * EPS32 * ref.abs() + TINY[torch.float32]


def torch_autograd_f64(G, Hs, Ws, S, std, mix_index, lam, dtype=torch.float64):
    """torch's own autograd of F.interpolate(bilinear, antialias=True) -> MixUp -> (v - 0.5) / std on the CPU in `dtype`:
    the gradient with respect to the source for the output gradient G (the source's values do not matter: linear)."""
    B = G.shape[0]
    x = torch.zeros(B, 3, Hs, Ws, dtype=dtype, requires_grad=True)
    v = F.interpolate(x, size=(S, S), mode="bilinear", antialias=True, align_corners=False)
    if mix_index is not None:
        lam_t = torch.tensor(_f32c(lam), dtype=dtype)
        v = lam_t * v + (1.0 - lam_t) * v[torch.as_tensor(mix_index).long()]
    out = (v - 0.5) / torch.tensor(_f32c(std), dtype=dtype)
    out.backward(G.to(dtype))
    return x.grad


def _axis_f32(S, n_in):
    """aa_axis / aa_w of csrc/preprocess.hip in torch fp32: W32 [S, in] with zeros outside each output's [lo, hi)."""
    f = torch.float32
    scale = torch.tensor(float(n_in), dtype=f) / torch.tensor(float(S), dtype=f)
    support = torch.clamp_min(scale, 1.0)
    invscale = torch.where(scale >= 1.0, 1.0 / scale, torch.ones((), dtype=f))
    i = torch.arange(S, dtype=f)
    center = scale * (i + 0.5)
    lo = (center - support + 0.5).trunc().clamp_min(0)
    hi = (center + support + 0.5).trunc().clamp_max(n_in)
    j = torch.arange(n_in, dtype=f)[None, :]
    x = ((j - center[:, None] + 0.5) * invscale).abs()
    raw = torch.where(x < 1.0, 1.0 - x, torch.zeros((), dtype=f))
    raw = raw * ((j >= lo[:, None]) & (j < hi[:, None]))
    total = torch.zeros(S, dtype=f)
    for k in range(n_in):                                  # the kernel's ascending fp32 sum
        total = total + raw[:, k]
    inv_total = torch.where(total != 0, 1.0 / total, torch.zeros((), dtype=f))
    return raw * inv_total[:, None]


def emulate_f32(G, Hs, Ws, S, std, mix_index, lam):
    """preprocess_bwd_kernel in torch fp32 on the CPU: the forward's fp32 weights, fp32 sums, the kernel's blend order."""
    f = torch.float32
    G = G.float()
    B = G.shape[0]
    if Hs == S and Ws == S:
        Fs = G
    else:
        Fs = _axis_f32(S, Hs).t() @ G @ _axis_f32(S, Ws)
    if mix_index is None:
        v = Fs
    else:
        lam_t = torch.tensor(lam, dtype=f)
        v = lam_t * Fs
        for j in range(B):
            v[int(mix_index[j])] += (1.0 - lam_t) * Fs[j]
    return v * (1.0 / torch.tensor(std, dtype=f))
