"""float64 reference of ``sgl_op_attn_probs`` with element-wise bounds derived from the number formats, the way
``tests/kernel_ref.py`` derives them.  A plain module: no tests, no fixtures.

The op computes, per (image, head, query i, key j), from operands already in the compute dtype and the fp32 ``lse`` it is
GIVEN (not re-derived, rows not renormalised):

    p_ij = exp(x_ij),   x_ij = S_ij * scale - lse_i,   S_ij = q_i . k_j,   scale = head_dim ** -0.5

The reference evaluates exactly that in float64 on the same operand values and the same fp32 lse.  Sources of error of the
kernels, all in fp32 (u = 2^-24 is the unit roundoff, EPS32 of kernel_ref):

* the score: head_dim products accumulated in fp32.  16-bit operands: the products are exact in fp32 and the matrix core
  adds them in an order of its own; fp32 operands: one rounding per fused multiply-add.  Either way
  |dS| <= head_dim u sum_d |q_d k_d|  (the classical bound for any summation order).
* the scale: the 16-bit kernels multiply by c = fl(fl(1 / sqrtf(dh)) * fl(log2 e)), three roundings; the fp32 kernels by
  fl(1 / sqrtf(dh)) (two) and round the product S * scale (one): 3 u |S scale| in both.
* the lse: the 16-bit kernels form -lse * fl(log2 e): two roundings, 2 u |lse|; the fp32 kernels subtract lse itself: 0.
* the final rounding of the exponent (the fused multiply-add's, or the subtraction's): u |x| (an error of the base-2
  exponent x log2 e by u |x log2 e| is one of x by u |x|).
  Together dx = scale head_dim u sum|q||k| + 3 u |S scale| + L u |lse| + u |x|,  L = 2 (16-bit) / 0 (fp32).
* the exponential: the hardware exp2 (16-bit kernels) and expf (fp32 kernels) are documented to 1 ulp: ULP32 = 2^-23
  relative (kernel_ref.HW_ULPS); a result below the smallest normal may be flushed: FLT_MIN absolute.

    bound(p) = p (expm1(dx) + ULP32) + FLT_MIN

HEAD_MEAN: the H values (the same fp32 p) are added in ascending head order starting from 0 (H - 1 roundings; the partial
sums of positive terms never exceed the total) and divided once by H (IEEE, one rounding): H u relative to the float64
mean of the fp32 FULL values.  No fitted constants anywhere.
"""
from __future__ import annotations

import torch

EPS32 = 2.0 ** -24
ULP32 = 2.0 ** -23
FLT_MIN = 2.0 ** -126
F32, BF16, BF16X3, F16 = 0, 1, 2, 3          # SGL_DTYPE_* the op takes
TORCH_DT = {F32: torch.float32, BF16: torch.bfloat16, BF16X3: torch.float32, F16: torch.float16}
DT_NAME = {F32: "f32", BF16: "bf16", BF16X3: "bf16x3", F16: "f16"}
FULL, HEAD_MEAN = 0, 1


def inputs(B, H, N, dh, dtype, seed=0, spread=1.0):
    """q, k [B, H, N, dh] in the operand dtype (CPU) and the fp32 lse of their float64 scores."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    tdt = TORCH_DT[dtype]
    q = (torch.randn(B, H, N, dh, generator=g) * spread).to(tdt)
    k = (torch.randn(B, H, N, dh, generator=g) * spread).to(tdt)
    S = (q.double() @ k.double().transpose(-1, -2)) * dh ** -0.5
    return q, k, torch.logsumexp(S, -1).float()


def pad_heads(x, DP):
    """[B, H, N, dh] -> head-major [B, H, N, DP] with zero pad columns (the layout the op reads)."""
    out = torch.zeros(*x.shape[:-1], DP, dtype=x.dtype)
    out[..., :x.shape[-1]] = x
    return out.contiguous()


def probs_ref(q, k, lse, dtype):
    """(p float64 [B, H, N, N], bound) for operands q, k [B, H, N, dh] (values of the operand dtype) and the fp32 lse
    [B, H, N] the op is given."""
    q64, k64, l64 = q.double(), k.double(), lse.double()
    dh = q.shape[-1]
    scale = dh ** -0.5
    S = (q64 @ k64.transpose(-1, -2)) * scale
    mag = (q64.abs() @ k64.abs().transpose(-1, -2)) * scale
    x = S - l64[..., None]
    p = torch.exp(x)
    n_lse = 0.0 if dtype in (F32, BF16X3) else 2.0
    dx = EPS32 * (dh * mag + 3 * S.abs() + n_lse * l64.abs()[..., None] + x.abs())
    return p, p * (torch.expm1(dx) + ULP32) + FLT_MIN


def head_mean_ref(full_f32):
    """(float64 mean over heads of the op's own fp32 FULL output [B, H, N, N], bound H u |mean|)."""
    H = full_f32.shape[1]
    m = full_f32.double().mean(1)
    return m, H * EPS32 * m.abs()


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound (inf where got is not finite)."""
    got = got.double()
    r = (got - ref).abs() / bound
    r = torch.where(torch.isfinite(got), r, torch.full_like(r, float("inf")))
    return float(r.max())
