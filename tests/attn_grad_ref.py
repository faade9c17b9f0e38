"""float64 reference of ``sgl_op_attn_grad_probs`` and ``sgl_op_pool_attn_grad_probs`` with element-wise bounds derived
from the number formats, built on ``attn_probs_ref.probs_ref``'s bound for P the way ``tests/kernel_ref.py`` derives
its bounds.  A plain module: no tests, no fixtures.

Per (image, head, query i, key j), from operands already in the compute dtype and the fp32 lse the op is GIVEN:

    dP_ij = sum_d dO_id V_jd          P_ij = exp(S_ij * scale - lse_i)  (attn_probs_ref)
    DP: dP      PDP: P * dP      RELEVANCE: relu(P * dP)

The reference evaluates exactly that in float64 on the same operand values.  Sources of error of the kernels, all in
fp32 (u = 2^-24 = EPS32):

* dP: head_dim products accumulated in fp32.  16-bit operands: a product of two 16-bit values (<= 11 significant bits
  each) is exact in fp32, and the matrix core adds head_dim (+ pad zeros) of them in an order of its own; fp32 operands:
  one rounding per fused multiply-add.  For any summation order of n terms the error is at most
  ((1 + u)^n - 1) sum|terms| <= (n + 1) u sum|terms| for n u < 0.01:
      b_dP = (head_dim + 1) u sum_d |dO_id| |V_jd|  +  head_dim * FLT_MIN
  (the last term: a product or partial sum below the smallest normal may be flushed to zero, FLT_MIN each).
* P: b_P of attn_probs_ref.probs_ref (same expression, same constants, same exp per route).
* PDP: the kernel forms fl(P^ * dP^) from its own P^ = P + eP, dP^ = dP + ed with |eP| <= b_P, |ed| <= b_dP:
      |P^ dP^ - P dP| <= b_P |dP| + (P + b_P) b_dP          (product rule, second-order term kept)
  plus the rounding of the product, u (P + b_P)(|dP| + b_dP), plus FLT_MIN for a flushed result.
* RELEVANCE: relu is 1-Lipschitz: |relu(a) - relu(b)| <= |a - b|, the PDP bound carries over unchanged, and the
  kernel's select (x > 0 ? x : 0) rounds nothing.
* HEAD_MEAN against the float64 mean of the exact values: the kernel adds its own fp32 per-head values x^_h in ascending
  head order from 0 (H - 1 roundings of partial sums, each at most sum_h |x^_h| in magnitude) and divides once by H
  (IEEE): at most H u (sum_h |x^_h|) / H of rounding on top of the mean of the per-head errors:
      b_mean = (sum_h b_h) / H  +  H u (sum_h (|x_h| + b_h)) / H
  For RELEVANCE (no sign changes) the second term is H u |mean| up to second order, the form the probs kernel's bound
  has; for the signed kinds the magnitudes do not cancel the way the values do, so the mean of magnitudes stands there.
  ``head_mean_of_full`` is the same statement against the kernel's OWN FULL output: only the H u term remains.

Pooling head: da_n = sum_d dO_d V_nd as one fp32 FMA chain over d (head_dim roundings: the dP bound with the operands
widened to fp32 first, exact for 16-bit V); p is the fp32 probability the forward stored, used as given, so b_P = 0 and
the product bound is p b_da + u p (|da| + b_da) + FLT_MIN.  No fitted constants anywhere.
"""
from __future__ import annotations

import torch

import attn_probs_ref as ar
from attn_probs_ref import EPS32, FLT_MIN, F32, BF16, BF16X3, F16, TORCH_DT, DT_NAME, FULL, HEAD_MEAN  # noqa: F401

DP, PDP, RELEVANCE = 0, 1, 2          # SGL_ATTN_GRAD_*
KINDS = (DP, PDP, RELEVANCE)
KIND_NAME = {DP: "dp", PDP: "pdp", RELEVANCE: "relevance"}


def inputs(B, H, N, dh, dtype, seed=0):
    """q, k, v, dout [B, H, N, dh] in the operand dtype (CPU) and the fp32 lse of the float64 scores."""
    q, k, lse = ar.inputs(B, H, N, dh, dtype, seed=seed)
    g = torch.Generator(device="cpu").manual_seed(seed + 7919)
    tdt = TORCH_DT[dtype]
    v = torch.randn(B, H, N, dh, generator=g).to(tdt)
    dout = torch.randn(B, H, N, dh, generator=g).to(tdt)
    return q, k, v, dout, lse


def token_major(x):
    """[B, H, N, dh] -> token-major [B*N, H*dh] (the layout of dout)."""
    B, H, N, dh = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * N, H * dh).contiguous()


def relu_keep_nan(x):
    return torch.where(x > 0, x, torch.where(x != x, x, torch.zeros_like(x)))


def dprobs_ref(v, dout):
    """(dP float64 [B, H, N, N], bound)."""
    v64, g64 = v.double(), dout.double()
    dh = v.shape[-1]
    dP = g64 @ v64.transpose(-1, -2)
    mag = g64.abs() @ v64.abs().transpose(-1, -2)
    return dP, (dh + 1) * EPS32 * mag + dh * FLT_MIN


def combine(kind, p, bp, dP, bd):
    """(value, bound) of one kind from P, dP and their bounds (module docstring)."""
    if kind == DP:
        return dP, bd
    x = p * dP
    b = bp * dP.abs() + (p + bp) * bd + EPS32 * (p + bp) * (dP.abs() + bd) + FLT_MIN
    return (x if kind == PDP else torch.clamp(x, min=0.0)), b


def grad_probs_ref(q, k, v, dout, lse, dtype, kind):
    """(x float64 [B, H, N, N], bound) of one kind, FULL."""
    dP, bd = dprobs_ref(v, dout)
    if kind == DP:
        return dP, bd
    p, bp = ar.probs_ref(q, k, lse, dtype)
    return combine(kind, p, bp, dP, bd)


def head_mean_ref(x, bound):
    """HEAD_MEAN reference and bound from the FULL float64 values and their bounds."""
    H = x.shape[1]
    return x.mean(1), bound.mean(1) + H * EPS32 * (x.abs() + bound).mean(1)


def head_mean_of_full(full_f32):
    """(float64 head mean of the op's own fp32 FULL output, bound H u mean_h |x_h|)."""
    H = full_f32.shape[1]
    f = full_f32.double()
    return f.mean(1), H * EPS32 * f.abs().mean(1) + FLT_MIN


def pool_ref(v, probs, dout, kind):
    """Pooling head: v [B, H, N, dh] operand dtype, probs fp32 [B, H, N], dout fp32 [B, H, dh] -> (x [B, H, N], bound)."""
    v64, g64, p = v.double(), dout.double(), probs.double()
    dh = v.shape[-1]
    da = torch.einsum("bhd,bhnd->bhn", g64, v64)
    mag = torch.einsum("bhd,bhnd->bhn", g64.abs(), v64.abs())
    bd = (dh + 1) * EPS32 * mag + dh * FLT_MIN
    return combine(kind, p, torch.zeros_like(p), da, bd)


def emulate_fp32(q, k, v, dout, lse, kind, mode):
    """What a kernel with fp32 accumulation computes, on the CPU: every product and sum in fp32."""
    dh = q.shape[-1]
    dP = dout.float() @ v.float().transpose(-1, -2)
    x = dP
    if kind != DP:
        S = q.float() @ k.float().transpose(-1, -2)
        p = torch.exp(S * torch.tensor(dh, dtype=torch.float32).rsqrt() - lse[..., None])
        x = p * dP
        if kind == RELEVANCE:
            x = relu_keep_nan(x)
    if mode == HEAD_MEAN:
        acc = torch.zeros_like(x[:, 0])
        for h in range(x.shape[1]):
            acc = acc + x[:, h]
        x = acc / float(x.shape[1])
    return x


def worst_ratio(got, ref, bound):
    return ar.worst_ratio(got, ref, bound)
