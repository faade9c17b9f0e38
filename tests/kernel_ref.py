"""float64 references, component-wise error bounds and CPU precision emulations for the per-kernel tests.

Every reference is the same operation in float64 by plain torch ops on the *rounded* inputs the kernel received, so only
accumulation order and output rounding differ.  Every bound is per element: ``|got - ref| <= bound`` for all elements
(`assert_within`), never one number per tensor.  Unit roundoffs: bf16 2^-8, fp16 2^-11, fp32 2^-24.

A bound is either derived from the number formats (the fp32-accumulation bound of a K-term sum in any order is
``K * 2^-24 * sum|terms|``), or it carries one constant that cannot be read off the code.  Those constants are set from
the CPU emulations below (the kernels' precision recipe written in torch fp32: what is rounded where, what is accumulated
in fp32) against float64, never from a kernel's output; tests/test_kernel_ref_host.py re-measures and asserts them:

  LN_C = 28     LayerNorm forward/backward: measured worst emulation/bound ratio with c = 1 over `ln_families` at D in
                {4, 64, 516, 1152, 2048}, 64 rows, three seeds: 6.94 for y (the tail of four or five fp32 roundings plus
                the wave-shaped sums; 4.4 to 6.9 by seed), 3.3 for the mean, 4.3 for rstd, 1.9 for dx; 6.94 x 4 = 27.8,
                rounded up to 28 (below the 64 at which the emulation itself would be suspect).
  ATTN_BWD_K = 2  attention backward: measured worst emulation/bound ratio with k = 1 is 0.86 (bf16 dV, inputs x 4) over
                `ATTN_EMU_SHAPES` at input scales 0.05, 1.2, 4 and 8 for both 16-bit types; times 2 gives 1.7, rounded
                up to 2.
  GELU term     not a constant: `gelu_eval_term` evaluates the kernel's formula in fp32 against float64 over the test's own
                pre-activations and takes the largest deviation times 4 (the hardware exp2/rcp may be an ulp or two worse
                than libm).  Over 2e5 N(0, 1.5) pre-activations it measures 1.9e-6 for gelu (half an ulp of |x| < 8, x 4) and
                7.7e-6 for its derivative (the formula's own 1 - s cancellation, amplified by x (2z)' <= 35, x 4).
  ADAMW_C = 2   AdamW (second half of the file, the kernels outside the encoder): the derived rounding counts times 2;
                measured worst emulation/bound with c = 1 is 0.74 (exp_avg), with c = 2 0.37.
  POS_BWD_C = 32  pos_resize_bwd (last part of the file, the kernels only the encoder calls): per-weight absolute error of
                the fp32 cubic polynomials in units of 2^-24; measured 11.6, times 2.76.
"""
import math

import torch

EPS32 = 2.0 ** -24
F32, BF16, BF16X3, F16 = 0, 1, 2, 3                      # SGL_DTYPE_* codes of include/siglip_hip.h
TORCH_DT = {F32: torch.float32, BF16: torch.bfloat16, BF16X3: torch.float32, F16: torch.float16}
UNIT = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
TINY = {torch.float32: 2.0 ** -150, torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25}   # half the smallest subnormal
DT_NAME = {F32: "f32", BF16: "bf16", BF16X3: "bf16x3", F16: "f16"}

LN_C = 28.0
ATTN_BWD_K = 2.0


# ---------------------------------------------------------------------------------------------------------------
# the metric
# ---------------------------------------------------------------------------------------------------------------
def worst_ratio(got, ref, bound):
    """max over elements of |got - ref| / bound (0/0 counts as 0; a non-finite `got` counts as inf)."""
    err = (got.double() - ref.double()).abs()
    r = err / bound.double().clamp_min(1e-300)
    r = torch.where(err == 0, torch.zeros_like(r), r)
    r = torch.where(torch.isfinite(got.double()), r, torch.full_like(r, float("inf")))
    return r.max().item() if r.numel() else 0.0


def assert_within(got, ref, bound, what):
    """Every element within its own bound; the message names the worst element."""
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    if got.numel() == 0:
        return 0.0
    err = (got.double() - ref.double()).abs()
    bad = ~(err <= bound.double())                       # NaN-safe: a NaN in `got` is a violation
    nbad = int(bad.sum().item())
    if nbad:
        r = torch.where(bad, err / bound.double().clamp_min(1e-300), torch.zeros_like(err))
        r = torch.nan_to_num(r, nan=float("inf"))
        i = int(r.argmax().item())
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), got.shape))
        raise AssertionError(f"{what}: {nbad} of {got.numel()} elements outside their bound; worst at {idx}: got "
                             f"{got.flatten()[i].item():.9g} ref {ref.flatten()[i].item():.9g} bound "
                             f"{bound.flatten()[i].item():.3g} (err/bound {r.flatten()[i].item():.3g})")
    return worst_ratio(got, ref, bound)


def rounding_bias(got, ref, u_out):
    """mean((|got| - |ref|) / (u_out |ref|)): 0 +- 0.01 for round-to-nearest over >= 1e4 elements, -0.72 for truncation."""
    got, ref = got.double().flatten(), ref.double().flatten()
    keep = ref.abs() > 1e-30
    assert int(keep.sum()) >= 10000, "rounding-bias statistic needs at least 1e4 elements"
    return (((got[keep].abs() - ref[keep].abs()) / (u_out * ref[keep].abs())).mean()).item()


def assert_rounding_unbiased(got, ref, u_out, what):
    b = rounding_bias(got, ref, u_out)
    assert abs(b) <= 0.05, f"{what}: rounding bias {b:+.3f} (round-to-nearest gives 0 +- 0.01, truncation -0.72)"
    return b


def truncate_to(x, dt):
    """Round toward zero to dtype `dt` (the mutant a component-wise bound has to catch), returned in dt."""
    x = x.float()
    if dt == torch.float32:
        return x
    r = x.to(dt).float()
    over = r.abs() > x.abs()
    toward_zero = torch.nextafter(r.to(dt), torch.zeros_like(r).to(dt))
    return torch.where(over, toward_zero.float(), r).to(dt)


# ---------------------------------------------------------------------------------------------------------------
# GEMM
# ---------------------------------------------------------------------------------------------------------------
def gemm_ref(A, B, K, u_out, adds=(), tiny_out=0.0):
    """ref = A @ B^T + sum(adds) in float64 and the fp32-accumulation bound
    u_out |ref| + (K + 4) 2^-24 (|A| @ |B|^T + sum |adds|): any summation order of K fp32 products, plus the bias /
    residual / position / alpha adds.  tiny_out (TINY of the output type) is the absolute rounding floor of an output in
    the subnormal range, where u_out |ref| no longer describes the format (fp16: 2^-25).
    Returns (ref, bound, bound without the output-rounding term)."""
    A64, B64 = A.double(), B.double()
    ref = A64 @ B64.t()
    mag = A64.abs() @ B64.abs().t()
    for t in adds:
        ref = ref + t.double()
        mag = mag + t.double().abs()
    acc_bound = (K + 4) * EPS32 * mag
    return ref, u_out * ref.abs() + tiny_out + acc_bound, acc_bound


def gelu64(x):
    x = x.double()
    return 0.5 * x * (1.0 + torch.tanh(0.7978845608028654 * (x + 0.044715 * x ** 3)))


def gelu_grad64(x):
    x = x.double()
    z = 0.7978845608028654 * (x + 0.044715 * x ** 3)
    t = torch.tanh(z)
    return 0.5 * (1.0 + t) + 0.5 * x * (1.0 - t * t) * 0.7978845608028654 * (1.0 + 3 * 0.044715 * x * x)


def _gelu_sigmoid_f32(x):
    """csrc/common.hip.h gelu_sigmoid in torch fp32: one exp2 and one reciprocal."""
    k1 = torch.tensor(-2.0 * 0.7978845608028654 * 1.4426950408889634, dtype=torch.float32)
    k2 = torch.tensor(-2.0 * 0.7978845608028654 * 0.044715 * 1.4426950408889634, dtype=torch.float32)
    e = torch.exp2(x * (k2 * (x * x) + k1))
    return 1.0 / (1.0 + e)


def gelu_f32_formula(x):
    x = x.float()
    return x * _gelu_sigmoid_f32(x)


def gelu_grad_f32_formula(x):
    x = x.float()
    s = _gelu_sigmoid_f32(x)
    zp = (6.0 * 0.7978845608028654 * 0.044715) * (x * x) + 2.0 * 0.7978845608028654
    return (x * (s * (1.0 - s))) * zp + s


def gelu_eval_term(pre, grad=False):
    """4 x the largest deviation of the kernel's fp32 formula from float64 over the pre-activations `pre` (evaluated at
    the fp32-rounded points, so the input rounding is not counted).  One number for the whole tensor."""
    x = pre.detach().float().cpu().flatten()
    if grad:
        d = (gelu_grad_f32_formula(x).double() - gelu_grad64(x)).abs().max()
    else:
        d = (gelu_f32_formula(x).double() - gelu64(x)).abs().max()
    return 4.0 * d.item()


def gemm_tn_ref(A, B, Mred, prior=None):
    """C = A^T @ B over Mred rows (+ prior for accumulate), fp32 out: 2^-24 |ref| + (Mred + 4) 2^-24 (|A|^T @ |B| + |prior|).
    Split-K needs no term of its own: partial sums added by atomics or from slabs are one more summation order of the
    same Mred products, and the bound holds for any order."""
    A64, B64 = A.double(), B.double()
    ref = A64.t() @ B64
    mag = A64.abs().t() @ B64.abs()
    if prior is not None:
        ref, mag = ref + prior.double(), mag + prior.double().abs()
    return ref, EPS32 * ref.abs() + (Mred + 4) * EPS32 * mag


# ---------------------------------------------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------------------------------------------
def ln_fwd_ref(x, gamma, beta, eps, u_out, c=LN_C, tiny_out=0.0):
    """float64 LayerNorm and its bounds: y, mean, rstd -> (ref, bound) each.
    y:    u_out |y| + c 2^-24 ((|x - mu| + |mu|) rstd |gamma| + |beta|)   (|mu|: the conditioning of the operation: the
          fp32 mean carries an error of order 2^-24 |mu| which rstd amplifies)
    (tiny_out: the absolute rounding floor of a subnormal 16-bit output, as in gemm_ref)
    mean: c 2^-24 mean|x|
    rstd: relative c 2^-24 + (c 2^-24 |mu| rstd)^2 / 2   (the error of the mean enters the variance squared)."""
    x64, g64, b64 = x.double(), gamma.double(), beta.double()
    mu = x64.mean(-1, keepdim=True)
    var = ((x64 - mu) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    y = (x64 - mu) * rstd * g64 + b64
    by = u_out * y.abs() + tiny_out + c * EPS32 * (((x64 - mu).abs() + mu.abs()) * rstd * g64.abs() + b64.abs())
    bmu = c * EPS32 * x64.abs().mean(-1)
    brs = rstd[:, 0] * (c * EPS32 + (c * EPS32 * mu[:, 0].abs() * rstd[:, 0]) ** 2 / 2)
    return (y, by), (mu[:, 0], bmu), (rstd[:, 0], brs)


def ln_bwd_ref(dy, x, mean, rstd, gamma, dres, u_lp, c=LN_C, tiny_out=0.0):
    """float64 LayerNorm backward from the SAME fp32 statistics the kernel is given.
    dx = rstd (g - mean(g) - h mean(g h)) [+ dres], g = dy gamma, h = (x - mean) rstd.
    bound(dx) = u |dx| + c 2^-24 (rstd (|g| + mean|g| + |h| mean|g h|) + |dres|);
    dgamma = sum_m dy h, dbeta = sum_m dy: (M/4 + 8) 2^-24 sum|terms| (any summation order of M fp32 terms)."""
    dy64, x64, g64 = dy.double(), x.double(), gamma.double()
    mu, rs = mean.double()[:, None], rstd.double()[:, None]
    M = x.shape[0]
    h = (x64 - mu) * rs
    g = dy64 * g64
    c1 = g.mean(-1, keepdim=True)
    c2 = (g * h).mean(-1, keepdim=True)
    dx = rs * (g - c1 - h * c2)
    mag = rs * (g.abs() + g.abs().mean(-1, keepdim=True) + h.abs() * (g * h).abs().mean(-1, keepdim=True))
    if dres is not None:
        dx = dx + dres.double()
        mag = mag + dres.double().abs()
    bdx32 = EPS32 * dx.abs() + c * EPS32 * mag
    bdxlp = u_lp * dx.abs() + tiny_out + c * EPS32 * mag
    t = dy64 * h
    k = (M / 4 + 8) * EPS32
    return (dx, bdx32, bdxlp), (t.sum(0), k * t.abs().sum(0)), (dy64.sum(0), k * dy64.abs().sum(0))


def _wave_sum_f32(s):
    """wave_sum of common.hip.h on [..., 64] fp32 lane partials: xor butterfly, every lane ends with the same total."""
    idx = torch.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        s = s + s[..., idx ^ off]
    return s[..., 0]


def _lanes(x, D):
    """[M, D] -> [M, V, 64, 4]: float4 number c = lane + 64 i of a row belongs to lane `lane`, slot i (zero padded)."""
    M = x.shape[0]
    nv = D // 4
    V = (nv + 63) // 64
    p = torch.zeros(M, V * 64, 4, dtype=torch.float32)
    p[:, :nv] = x.float().view(M, nv, 4)
    return p.view(M, V, 64, 4), nv


def ln_fwd_emulate(x, gamma, beta, eps, out_dt):
    """ln_fwd_kernel in torch fp32 on the CPU: two passes, per-lane partial sums over the lane's float4s, wave butterfly."""
    M, D = x.shape
    v, nv = _lanes(x, D)
    live = (torch.arange(v.shape[1] * 64).view(v.shape[1], 64) < nv)[None, :, :, None]
    invD = torch.tensor(1.0 / D, dtype=torch.float32)
    s = torch.zeros(M, 64)
    for i in range(v.shape[1]):
        s = s + ((v[:, i, :, 0] + v[:, i, :, 1]) + (v[:, i, :, 2] + v[:, i, :, 3]))
    mu = _wave_sum_f32(s) * invD
    d = torch.where(live, v - mu[:, None, None, None], torch.zeros(()))
    q = torch.zeros(M, 64)
    for i in range(v.shape[1]):
        for j in range(4):
            q = q + d[:, i, :, j] * d[:, i, :, j]
    rs = 1.0 / torch.sqrt(_wave_sum_f32(q) * invD + torch.tensor(eps, dtype=torch.float32))
    y = (x.float() - mu[:, None]) * rs[:, None] * gamma.float() + beta.float()
    return y.to(out_dt), mu, rs


def ln_bwd_emulate(dy, x, mean, rstd, gamma, dres, lp_dt):
    """ln_bwd_kernel in torch fp32 on the CPU (same lane-shaped sums); dgamma/dbeta as plain fp32 row-order sums."""
    M, D = x.shape
    dyf = dy.float()
    mu, rs = mean.float()[:, None], rstd.float()[:, None]
    h = (x.float() - mu) * rs
    g = dyf * gamma.float()
    gl, _ = _lanes(g, D)
    ghl, _ = _lanes(g * h, D)
    c1 = torch.zeros(M, 64)
    c2 = torch.zeros(M, 64)
    for i in range(gl.shape[1]):
        for j in range(4):
            c1 = c1 + gl[:, i, :, j]
            c2 = c2 + ghl[:, i, :, j]
    invD = torch.tensor(1.0 / D, dtype=torch.float32)
    c1 = (_wave_sum_f32(c1) * invD)[:, None]
    c2 = (_wave_sum_f32(c2) * invD)[:, None]
    dx = rs * (g - c1 - h * c2)
    if dres is not None:
        dx = dx + dres.float()
    t = dyf * h
    dg = torch.zeros(D)
    db = torch.zeros(D)
    for m in range(M):
        dg = dg + t[m]
        db = db + dyf[m]
    return dx, dx.to(lp_dt), dg, db


def ln_families(M, D, seed=0, device="cpu"):
    """The LayerNorm input families: name -> x [M, D] fp32."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    fam = {
        "gauss": rn(M, D) * 2 + 0.3,
        "mean1000": rn(M, D) + 1000.0,
        "const_exact": torch.full((M, D), 0.5),
        "const_inexact": torch.full((M, D), 1000.1),
        "zeros": torch.zeros(M, D),
    }
    out = rn(M, D)
    out[:, D // 3] *= 300.0
    fam["outlier"] = out
    return {k: v.to(device) for k, v in fam.items()}


# ---------------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------------
def attn_ref(q, k, v, dout=None):
    """float64 attention on [..., N, dh] tensors.  Returns a dict with O, lse, P, S-scale and (with dout) dQ, dK, dV, dS."""
    q, k, v = q.double(), k.double(), v.double()
    dh = q.shape[-1]
    scale = dh ** -0.5
    S = (q @ k.transpose(-1, -2)) * scale
    lse = torch.logsumexp(S, dim=-1)
    P = torch.exp(S - lse[..., None])
    O = P @ v
    r = dict(q=q, k=k, v=v, scale=scale, P=P, O=O, lse=lse)
    if dout is not None:
        dO = dout.double()
        dP = dO @ v.transpose(-1, -2)
        delta = (dO * O).sum(-1, keepdim=True)
        dS = P * (dP - delta)
        r.update(dO=dO, dS=dS, dV=P.transpose(-1, -2) @ dO, dK=scale * dS.transpose(-1, -2) @ q, dQ=scale * dS @ k)
    return r


def _score_rel(r, N):
    """eps_S per query: the relative move of P from the fp32 error of the scores,
    scale (dh + 2) 2^-24 max_j(|q_i| . |k_j|)."""
    dh = r["q"].shape[-1]
    qk = r["q"].abs() @ r["k"].abs().transpose(-1, -2)
    return r["scale"] * (dh + 2) * EPS32 * qk.max(-1, keepdim=True).values


def attn_fwd_bound(r, u, fp32_mode=False):
    """u |O| + 2u (P @ |V|) + N 2^-25 max|V| + 2 eps_S (P @ |V|)   (16-bit operand kernels: P is rounded to the operand
    type before P.V while l is summed unrounded; the factor 2 covers fp32 accumulation and the exp2 approximation; the third
    term is fp16's subnormal floor for tiny P).
    fp32 modes (SGL_DTYPE_F32 and SGL_DTYPE_BF16X3, u = 2^-24): nothing is rounded to 16 bits, so the P.V product takes the
    fp32-accumulation form (N + 4) 2^-24 (P @ |V|) in place of the subnormal-floor term.  The split-bf16 residual
    3 * 2^-24 was not needed anywhere: BF16X3 attention runs whole fp32 operands on the fp32 MFMA, and the single-kernel
    GEMM entry points have no split-operand path (dtype BF16X3 there runs the strict fp32 kernel).
    lse: 2^-20 (1 + |lse|) absolute."""
    N = r["P"].shape[-1]
    PV = r["P"] @ r["v"].abs()
    eS = _score_rel(r, N)
    b = u * r["O"].abs() + 2 * u * PV + 2 * eS * PV
    if fp32_mode:
        b = b + (N + 4) * EPS32 * PV
    else:
        b = b + N * 2.0 ** -25 * r["v"].abs().max()
    return b, 2.0 ** -20 * (1 + r["lse"].abs())


def attn_bwd_bound(r, u, k=ATTN_BWD_K, fp32_mode=False, tiny=0.0):
    """dV: k u (P^T @ |dO|); dK: k u scale (|dS|^T @ |Q|); dQ: k u scale (|dS| @ |K|); each plus the output rounding
    u |ref|, plus the relative move `rel` of P (2 eps_S from the scores and the lse bound 2^-20 (1 + |lse|): the backward
    rebuilds P from the stored fp32 lse) through the same absolute-value products, plus delta built from the forward's
    rounded output, u P rowsum(|dO| |O|), through the dK / dQ products.
    `tiny` (half the operand type's smallest subnormal, TINY) is the absolute floor of rounding P and dS (dS already
    carries `scale`), the backward's counterpart of the forward's N 2^-25 max|V|: N tiny max|dO|, N tiny max|Q|, N tiny
    max|K|.  It matters for fp16 with a peaked softmax (most of P is below 2^-24).
    dS = P (dP - delta) cancels: the fp32 sums dP and delta carry (dh + 4) 2^-24 (|dO| @ |V|^T + rowsum(|dO| |O|)) each,
    absolute, which P carries into dS whatever is left of dP - delta (negligible next to k u |dS| for 16-bit operands, the
    leading term in the fp32 modes).
    fp32 modes: k u is replaced by the fp32-accumulation factor (N + 4) 2^-24."""
    N = r["P"].shape[-1]
    P, dS, dO, sc = r["P"], r["dS"].abs(), r["dO"].abs(), r["scale"]
    rel = 2 * _score_rel(r, N) + 2.0 ** -20 * (1 + r["lse"].abs()[..., None])
    f = (N + 4) * EPS32 if fp32_mode else k * u
    dlt = P * (u * (dO * r["O"].abs()).sum(-1, keepdim=True))
    dh = r["q"].shape[-1]
    cancel = P * ((dh + 4) * EPS32 * (dO @ r["v"].abs().transpose(-1, -2) + (dO * r["O"].abs()).sum(-1, keepdim=True)))
    dSe = f * dS + rel * dS + dlt + cancel
    Pe = f * P + rel * P
    bV = u * r["dV"].abs() + Pe.transpose(-1, -2) @ dO + N * tiny * dO.max()
    bK = u * r["dK"].abs() + sc * dSe.transpose(-1, -2) @ r["q"].abs() + N * tiny * r["q"].abs().max()
    bQ = u * r["dQ"].abs() + sc * dSe @ r["k"].abs() + N * tiny * r["k"].abs().max()
    return bQ, bK, bV


LOG2E = 1.4426950408889634
ATTN_EMU_SHAPES = [(729, 72), (130, 32), (300, 64), (65, 96), (1024, 40)]


def attn_emulate(q, k, v, dout, dt, rnd=None):
    """The attention kernels' precision recipe in torch fp32 on the CPU, one head ([N, dh] operands already in `dt`):
    forward = 64-key online softmax in the exp2 domain, P rounded to `dt` before P.V, l summed unrounded, fp32 accumulate,
    output rounded; backward = P rebuilt from the fp32 lse, delta from the ROUNDED output, dS = P (dP scale - delta scale)
    with P and dS rounded to `dt` before their products, fp32 accumulate, outputs rounded.
    rnd(x) overrides the rounding to `dt` (the truncating mutant)."""
    rnd = rnd or (lambda x: x.to(dt))
    qf, kf, vf, dOf = q.float(), k.float(), v.float(), dout.float()
    N, dh = qf.shape
    scale = torch.tensor(dh ** -0.5, dtype=torch.float32)
    c = scale * torch.tensor(LOG2E, dtype=torch.float32)
    m = torch.full((N,), -float("inf"))
    l = torch.zeros(N)
    o = torch.zeros(N, dh)
    for t0 in range(0, N, 64):
        S = qf @ kf[t0:t0 + 64].t()
        m_new = torch.maximum(m, S.max(-1).values)
        alpha = torch.exp2(c * (m - m_new))
        p = torch.exp2(S * c - (m_new * c)[:, None])
        l = l * alpha + p.sum(-1)
        o = o * alpha[:, None] + rnd(p).float() @ vf[t0:t0 + 64]
        m = m_new
    O = rnd(o / l[:, None])
    lse = m * scale + torch.log(l)
    Lq = -lse * torch.tensor(LOG2E, dtype=torch.float32)
    nds = -(dOf * O.float()).sum(-1) * scale
    S = qf @ kf.t()
    p = torch.exp2(S * c + Lq[:, None])
    dP = dOf @ vf.t()
    dS = p * (dP * scale + nds[:, None])
    pr, dSr = rnd(p).float(), rnd(dS).float()
    return O, lse, rnd(dSr @ kf), rnd(dSr.t() @ qf), rnd(pr.t() @ dOf)


def attn_inputs(kind, B, H, N, dh, tdt, seed=0, jump_key=None):
    """q, k, v, dout as [B, H, N, dh] tensors of dtype tdt (CPU).  kinds:
    gauss      N(0, 1.2);
    jump       one key far above the rest for one query (score 128), at key index `jump_key`: the running max jumps there;
    peaked     q, k scaled (x 16, still far inside fp16 range) so that the softmax is one-hot to fp32 precision;
    positive   gauss q, k with v, dout > 0: nothing cancels in P.V and P^T.dO, for the rounding-bias statistic;
    flat       scale 0.01: a near-uniform softmax;
    offset     all scores shifted by a common +60 through one constant component of q and k."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    q, k, v, do = rn(B, H, N, dh), rn(B, H, N, dh), rn(B, H, N, dh), rn(B, H, N, dh)
    if kind == "gauss":
        q, k, v = q * 1.2, k * 1.2, v * 1.2
    elif kind == "jump":
        q, k, v = q * 0.5, k * 0.5, v * 0.5
        a = math.sqrt(128.0 * math.sqrt(dh) / dh)        # a*a*dh / sqrt(dh) = 128
        q[:, :, min(7, N - 1)] = a
        k[:, :, jump_key] = a
    elif kind == "peaked":
        q, k = q * 16.0, k * 16.0                        # scores ~ N(0, 256^2): the top two of a row are ~70 apart, far more
                                                         # than ln 2^24 = 16.6, so most rows are one-hot in fp32
    elif kind == "positive":
        q, k, v, do = q * 1.2, k * 1.2, v.abs() + 0.5, do.abs() + 0.5
    elif kind == "flat":
        q, k = q * 0.01, k * 0.01
    elif kind == "offset":
        a = math.sqrt(60.0 * math.sqrt(dh))              # q[0] * k[0] / sqrt(dh) = 60
        q[..., 0] = a
        k[..., 0] = a
    else:
        raise ValueError(kind)
    return tuple(t.to(tdt) for t in (q, k, v, do))


# ---------------------------------------------------------------------------------------------------------------
# small ops
# ---------------------------------------------------------------------------------------------------------------
def colsum_ref(x, M, prior=None):
    """float64 column sums and the bound (M/4 + 8) 2^-24 colsum|x| (+ the prior for accumulate)."""
    x64 = x.double()
    ref, mag = x64.sum(0), x64.abs().sum(0)
    if prior is not None:
        ref, mag = ref + prior.double(), mag + prior.double().abs()
    return ref, (M / 4 + 8) * EPS32 * mag


def pos_resize_ref(table, g0, gh, gw):
    """float64 F.interpolate(bicubic, align_corners=False, no antialias) of a [g0*g0, D] table -> [gh*gw, D], as
    oracle/siglip_oracle.py and the HF interpolate_pos_encoding do."""
    D = table.shape[1]
    t = table.double().view(1, g0, g0, D).permute(0, 3, 1, 2)
    o = torch.nn.functional.interpolate(t, size=(gh, gw), mode="bicubic", align_corners=False)
    return o.permute(0, 2, 3, 1).reshape(gh * gw, D)


def pos_resize_bound(table, g0):
    """Per channel d: (2 g0 + 24) 2^-24 * 1.375^2 * max|table[:, d]|.  1.375 is the largest sum of |cubic weights|
    (A = -0.75, t = 0.5) per axis; the source coordinate scale (o + 0.5) - 0.5 carries up to 2 g0 2^-24 absolute error
    over both axes, which the weights (slope <= 1) pass on; 16 products and adds and the weight polynomials are the 24."""
    return ((2 * g0 + 24) * EPS32 * 1.375 ** 2) * table.double().abs().max(0).values


# ===============================================================================================================
# kernels outside the encoder (csrc/preprocess.hip, video_tail.hip, decoder.hip, decoder_tail.hip, optimizer.hip)
#
# Every bound below is derived: output rounding UNIT / TINY, fp32 accumulation from the number of addends the element
# has (a sum of n fp32 terms in any order is off by at most n 2^-24 sum|terms|; where the kernel's order is fixed by the
# code, n is the depth of that order: the per-thread strided chain plus the 6 butterfly stages and 2 LDS adds of a
# 256-thread block), and explicit terms for the hardware approximations:
#   V_EXP_F32 and V_RCP_F32 (`__builtin_amdgcn_exp2f`, `__builtin_amdgcn_rcpf`, and `__expf` = exp2(x log2 e)): 1 ulp
#       each (the accuracy the public CDNA3 / CDNA4 ISA guides state for both instructions; no copy of the guide ships
#       with the toolchain, so the figure is quoted, not read off a local file);  HW_ULPS = 1.
#   V_RCP_F32 may flush a subnormal RESULT to zero, so a sigmoid below 2^-126 carries the absolute floor 2^-126.
#   plain `/` and sqrtf: 2.5 ulp and 1 ulp at the worst (hipcc's default is correctly rounded; 2.5 ulp is the OpenCL
#       figure the device library guarantees without that flag);  log1pf: 2 ulp (OCML's stated accuracy).
# One constant is fitted, by the convention at the top of this file: ADAMW_C = 2 (see adamw_ref).  tests/
# test_kernel_ref_host.py runs an fp32 emulation of every operation against its bound and asserts the worst ratio is at
# most 0.5 for fp32 outputs (a 16-bit store alone reaches its own half-ulp term, so those are held to 1); the measured
# ratios are listed there next to each assertion.
# ===============================================================================================================
ULP32 = 2.0 ** -23
HW_ULPS = 1.0                    # V_EXP_F32 / V_RCP_F32
DIV_ULPS, SQRT_ULPS, LOG1P_ULPS = 2.5, 1.0, 2.0
FLT_MIN = 2.0 ** -126
BLOCK_TREE = 8                   # wave_sum's 6 butterfly stages + (r0 + r1) + (r2 + r3)
NV = {F32: 4, BF16: 8}


def _f32c(x):
    """The float32 rounding of a Python scalar, as a Python float (what the kernel receives for a `float` argument)."""
    return torch.tensor(x, dtype=torch.float32).item()


# ---- gate_mul --------------------------------------------------------------------------------------------------
def sigmoid_fast_ref(z):
    """float64 sigmoid(z) and the bound of `sigmoidf_fast` = rcp(1 + exp2(fl(-z L))), L = fl(log2 e):
    the exponent fl(-z L) is off by 2 * 2^-24 |z| log2 e (L's rounding and the product's), i.e. exp2 by the RELATIVE
    2 * 2^-24 |z|: the bound grows with |z|; V_EXP_F32 adds HW_ULPS ulp.  s = 1 / (1 + e) passes a relative error of e on
    with the factor (1 - s); the add rounds once (2^-24) and V_RCP_F32 adds HW_ULPS ulp.  Absolute floor 2^-126: the
    result of V_RCP_F32 may be flushed when subnormal, and exp2 overflows to inf (s = 0) only where s < 2^-126."""
    z = z.double()
    s = torch.sigmoid(z)
    rel_e = 2 * EPS32 * z.abs() + HW_ULPS * ULP32
    rel_s = (1 - s) * rel_e + EPS32 + HW_ULPS * ULP32
    return s, s * rel_s * (1 + 1e-3) + FLT_MIN


def gate_mul_ref(g, x, out_dt):
    """y = sigmoid(g) x: bound = |x| err(s) + 2^-24 |y| (the product) + UNIT |y| + TINY (the store)."""
    s, es = sigmoid_fast_ref(g)
    x = x.double()
    y = s * x
    return y, x.abs() * es + (EPS32 + UNIT[out_dt]) * y.abs() + TINY[out_dt]


def gate_mul_bwd_ref(dy, g, x, out_dt):
    """dx = dy s;  dg = dy x (s (1 - s)).  fl(1 - s) is off by err(s) + 2^-24 (1 - s), so s (1 - s) by
    (1 - s) err(s) + s (err(s) + 2^-24 (1 - s)) + 2^-24 s (1 - s) <= err(s) + 2 * 2^-24 s (1 - s); two more products."""
    s, es = sigmoid_fast_ref(g)
    d, x = dy.double(), x.double()
    dx = d * s
    dg = d * x * (s * (1 - s))
    bdx = d.abs() * es + (EPS32 + UNIT[out_dt]) * dx.abs() + TINY[out_dt]
    bdg = (d * x).abs() * (es + 2 * EPS32 * s * (1 - s)) + (2 * EPS32 + UNIT[out_dt]) * dg.abs() + TINY[out_dt]
    return (dg, bdg), (dx, bdx)


def gate_mul_emulate(g, x, dy, out_dt):
    """The kernels in torch fp32 on the CPU (torch.exp2 and a true division standing in for the two builtins)."""
    L = torch.tensor(LOG2E, dtype=torch.float32)
    gf, xf, df = g.float(), x.float(), dy.float()
    s = 1.0 / (1.0 + torch.exp2(-gf * L))
    return (s * xf).to(out_dt), ((df * xf) * (s * (1.0 - s))).to(out_dt), (df * s).to(out_dt)


GATE_SWEEP = [0.0, 1e-3, -1e-3, 20.0, -20.0, 88.0, -88.0, 104.0, -104.0, 200.0, -200.0]


# ---- depthwise 3x3 ---------------------------------------------------------------------------------------------
def _shift(x, dy, dx):
    """x [B, gh, gw, E] -> the tensor whose (y, x) entry is x(y + dy - 1, x + dx - 1), zeros outside."""
    B, gh, gw, E = x.shape
    p = torch.zeros(B, gh + 2, gw + 2, E, dtype=x.dtype, device=x.device)
    p[:, 1:gh + 1, 1:gw + 1] = x
    return p[:, dy:dy + gh, dx:dx + gw]


def dwconv_ref(x, w9, bias, flip, out_dt):
    """y[b,y,x,e] = bias[e] + sum_k w9[k or 8 - k][e] x[b, y + k/3 - 1, x + k%3 - 1, e] in float64 on channels-last data;
    bound = (UNIT |y| + TINY) + (n + 1) 2^-24 (sum |w x| + |bias|), n = the in-range taps of THAT pixel (an fma chain of
    n links on top of the bias)."""
    x64, w64 = x.double(), w9.double()
    ones = torch.ones_like(x64[..., :1])
    y = torch.zeros_like(x64)
    mag = torch.zeros_like(x64)
    n = torch.zeros_like(ones)
    for k in range(9):
        wk = w64[8 - k if flip else k]
        xs = _shift(x64, k // 3, k % 3)
        y = y + wk * xs
        mag = mag + (wk * xs).abs()
        n = n + _shift(ones, k // 3, k % 3)
    if bias is not None:
        y = y + bias.double()
        mag = mag + bias.double().abs()
    return y, UNIT[out_dt] * y.abs() + TINY[out_dt] + (n + 1) * EPS32 * mag


def dwconv_wgrad_ref(x, dy, prior=None):
    """dw10[k][e] = sum_pixels x(shifted by tap k) dy, row 9 = sum dy (+ prior), fp32 out: 2^-24 |ref| +
    (npix + 4) 2^-24 (sum |x dy| + |prior|): any order of the npix products (block partials, lanes, the fold)."""
    x64, d64 = x.double(), dy.double()
    E = x.shape[-1]
    npix = x64.numel() // E
    rows, mags = [], []
    for k in range(9):
        t = _shift(x64, k // 3, k % 3) * d64
        rows.append(t.reshape(-1, E).sum(0))
        mags.append(t.abs().reshape(-1, E).sum(0))
    rows.append(d64.reshape(-1, E).sum(0))
    mags.append(d64.abs().reshape(-1, E).sum(0))
    ref, mag = torch.stack(rows), torch.stack(mags)
    if prior is not None:
        ref, mag = ref + prior.double(), mag + prior.double().abs()
    return ref, EPS32 * ref.abs() + (npix + 4) * EPS32 * mag


# ---- l2norm + temporal mean ------------------------------------------------------------------------------------
def _block_depth(n):
    """Depth of a 256-thread block's sum of n terms: each thread's strided chain, then BLOCK_TREE tree adds."""
    return math.ceil(n / 256) + BLOCK_TREE


def l2norm_tmean_fwd_ref(f, B, T):
    """out[b] = mean_t f_t / |f_t|, inv_norm = 1 / |f_t|.
    inv_norm: the squared norm is a sum of D positive squares (one rounding each, depth `_block_depth(D)`), relative
    (depth + 1) 2^-24; a square in the subnormal range rounds by 2^-150 absolute instead, D 2^-150 in all: the bound says
    what is promised for a row of norm 1e-18 (squares near 2^-126).  A row of norm 1e18 has squares of 1e34 and needs no
    term.  sqrt and `/` halve / add: rel(inv) = (depth + 1) 2^-25 + D 2^-151 / sumsq + (SQRT_ULPS + DIV_ULPS) ulp.
    out: T products f inv (rel(inv) + 2^-24 each), T adds, the final * (1 / T) (two roundings)."""
    D = f.shape[-1]
    f64 = f.double().view(B, T, D)
    ss = (f64 * f64).sum(-1)
    inv = 1.0 / torch.sqrt(ss)
    rel = (_block_depth(D) + 1) * EPS32 / 2 + D * 2.0 ** -151 / ss + (SQRT_ULPS + DIV_ULPS) * ULP32
    out = (f64 * inv[..., None]).mean(1)
    mag = (f64.abs() * (inv * (rel + (T + 3) * EPS32))[..., None]).sum(1) / T
    return (out, mag + EPS32 * out.abs() + TINY[torch.float32]), (inv.reshape(-1), (inv * rel).reshape(-1))


def l2norm_tmean_bwd_ref(f, inv_norm, dout, B, T):
    """df_t = (g - f_t inv (f_t . g) inv) inv / T from the SAME fp32 inv_norm the kernel is given.
    dot = (f . g) inv: depth(D) 2^-24 sum|f g| inv + 2 * 2^-24 |dot|;  df: k (4 * 2^-24 (|g| + |f| inv |dot|) +
    |f| inv err(dot)), k = inv / T (its rounding and the `/` are two of the four)."""
    D = f.shape[-1]
    f64, inv = f.double().view(B, T, D), inv_norm.double().view(B, T, 1)
    g = dout.double().view(B, 1, D)
    raw = (f64 * g).sum(-1, keepdim=True)
    dot = raw * inv
    edot = (_block_depth(D) + 1) * EPS32 * (f64 * g).abs().sum(-1, keepdim=True) * inv + 2 * EPS32 * dot.abs()
    k = inv / T
    df = (g - f64 * inv * dot) * k
    mag = g.abs() + f64.abs() * inv * dot.abs()
    bound = k * ((4 + DIV_ULPS * 2) * EPS32 * mag + f64.abs() * inv * edot) + EPS32 * df.abs() + TINY[torch.float32]
    return df.reshape(B * T, D), bound.reshape(B * T, D)


def l2norm_emulate(f, dout, B, T):
    """Both kernels in torch fp32: per-thread strided sums, wave butterfly, four-wave fold."""
    D = f.shape[-1]
    ff = f.float().view(B * T, D)

    def block_sum(v):                                     # [rows, D] -> [rows]
        pad = torch.zeros(v.shape[0], math.ceil(D / 256) * 256)
        pad[:, :D] = v
        s = torch.zeros(v.shape[0], 256)
        for i in range(pad.shape[1] // 256):
            s = s + pad[:, i * 256:(i + 1) * 256]
        w = _wave_sum_f32(s.view(-1, 4, 64))
        return (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])
    inv = 1.0 / torch.sqrt(block_sum(ff * ff))
    acc = torch.zeros(B, D)
    fv = (ff * inv[:, None]).view(B, T, D)
    for t in range(T):
        acc = acc + fv[:, t]
    out = acc * torch.tensor(1.0 / T, dtype=torch.float32)
    g = dout.float().repeat_interleave(T, 0)
    dot = block_sum(ff * g) * inv
    k = inv / torch.tensor(float(T))
    df = (g - ff * inv[:, None] * dot[:, None]) * k[:, None]
    return out, inv, df


# ---- seg_loss --------------------------------------------------------------------------------------------------
def _bilinear_axis(g, S):
    """align_corners=False source positions of S outputs on g inputs with the kernel's fp32 scale fl(g) / fl(S):
    W [S, g] interpolation matrix, Dm [S, g] = |d W / d position| (one at each of the two taps, zero where they
    coincide), all float64."""
    scale = (torch.tensor(float(g), dtype=torch.float32) / torch.tensor(float(S), dtype=torch.float32)).double()
    i = torch.arange(S, dtype=torch.float64)
    s = (scale * (i + 0.5) - 0.5).clamp_min(0.0)
    i0 = s.floor().clamp_max(g - 1).long()
    i1 = (i0 + 1).clamp_max(g - 1)
    w1 = s - i0.double()
    W = torch.zeros(S, g, dtype=torch.float64)
    Dm = torch.zeros(S, g, dtype=torch.float64)
    r = torch.arange(S)
    W[r, i0] += 1.0 - w1
    W[r, i1] += w1
    Dm[r, i0] -= 1.0
    Dm[r, i1] += 1.0
    return W, Dm


def seg_pixels_ref(lr, tgt):
    """Per output pixel, float64: z, its bound, p, its bound, bce, its bound.  lr [B, g, g], tgt [B, S, S] (CPU).
    z = W L W^T.  The fp32 source position fl(fl(scale (i + 0.5)) - 0.5) is off by cs = 3 * 2^-24 g at the most (the two
    roundings at magnitude <= g, and the clamp / floor keep z continuous), which moves z by cs (|dz/dy| + |dz/dx|), the
    slopes being differences of neighbouring logits; the three lerps round 6 times on |W| |L| |W|^T.
    e = __expf(-|z|) = V_EXP_F32(fl(-|z| log2 e)): relative 2 * 2^-24 |z| + HW_ULPS ulp.
    p = 1 / (1 + e) or e / (1 + e): (1 - p) rel(e) + 2^-24 + DIV_ULPS ulp relative, plus p (1 - p) err(z).
    bce = max(z, 0) - z t + log1pf(e): |p - t| err(z) + 2 * 2^-24 (|z| + |z t|) + LOG1P_ULPS ulp log1p(e) + e rel(e)
    + 2 * 2^-24 |bce| (the two adds)."""
    g, S = lr.shape[-1], tgt.shape[-1]
    W, Dm = _bilinear_axis(g, S)
    L, t = lr.double(), tgt.double()
    z = W @ L @ W.t()
    cs = 3 * EPS32 * g
    slope = (Dm @ L @ W.t()).abs() + (W @ L @ Dm.t()).abs()
    ez = cs * slope + 6 * EPS32 * (W @ L.abs() @ W.t())
    p = torch.sigmoid(z)
    e = torch.exp(-z.abs())
    rel_e = 2 * EPS32 * z.abs() + HW_ULPS * ULP32
    ep = p * ((1 - p) * rel_e + EPS32 + DIV_ULPS * ULP32) + p * (1 - p) * ez + TINY[torch.float32]
    bce = z.clamp_min(0) - z * t + torch.log1p(e)
    ebce = (p - t).abs() * ez + 2 * EPS32 * (z.abs() + (z * t).abs()) + LOG1P_ULPS * ULP32 * torch.log1p(e) + \
        e * rel_e + 2 * EPS32 * bce.abs()
    return dict(z=z, ez=ez, p=p, ep=ep, bce=bce, ebce=ebce, t=t, W=W, Dm=Dm, cs=cs)


def seg_loss_fwd_ref(lr, tgt):
    """partial[b][chunk][4] = {sum bce, sum p t, sum p, sum t} over 8 output rows: the per-pixel bounds summed, plus the
    fixed-order accumulation (8 ceil(S / 256) + BLOCK_TREE) 2^-24 sum|terms| (+ one product rounding for p t)."""
    r = seg_pixels_ref(lr, tgt)
    B, S = tgt.shape[0], tgt.shape[-1]
    chunks = (S + 7) // 8
    depth = 8 * math.ceil(S / 256) + BLOCK_TREE
    terms = torch.stack([r["bce"], r["p"] * r["t"], r["p"], r["t"]], -1)              # [B, S, S, 4]
    errs = torch.stack([r["ebce"], r["t"] * r["ep"] + EPS32 * r["p"] * r["t"], r["ep"], torch.zeros_like(r["t"])], -1)
    ref = torch.zeros(B, chunks, 4, dtype=torch.float64)
    bound = torch.zeros(B, chunks, 4, dtype=torch.float64)
    for c in range(chunks):
        sl = slice(8 * c, min(8 * c + 8, S))
        ref[:, c] = terms[:, sl].sum((1, 2))
        bound[:, c] = errs[:, sl].sum((1, 2)) + depth * EPS32 * terms[:, sl].abs().sum((1, 2))
    return ref, bound


def seg_loss_bwd_ref(lr, tgt, sums, coef, eps):
    """dlogits_lr = W^T dz W (the transposed interpolation, written out), dz = c_bce (p - t) + c_dice p (1 - p) F,
    F = (2 t D - 2 I) / D^2, I = sums[1], D = sums[2] + sums[3] + eps from the SAME fp32 sums / coef / eps the kernel reads.
    F: D rounds twice, 1 / (D D) rounds twice more plus DIV_ULPS ulp, the difference cancels: (8 * 2^-24 + DIV_ULPS ulp)
    (|2 t D| + |2 I|) / D^2.  err(dz) = |c_bce| (err(p) + 2^-24 |p - t|) + |c_dice| (err(p) |F| + p (1 - p) (err(F) +
    4 * 2^-24 |F|)) + 2 * 2^-24 |dz|.
    Gather: W^T err(dz) W, plus the weights' own position error cs on either axis (|Dm|^T |dz| W + W^T |dz| |Dm|), plus
    the accumulation over the rows and columns that feed one low-res pixel, (rows + cols + 8) 2^-24 W^T |dz| W."""
    r = seg_pixels_ref(lr, tgt)
    p, t, W, Dm = r["p"], r["t"], r["W"], r["Dm"].abs()
    s64, c64 = sums.double(), coef.double()
    cb, cd = c64[:, 0, None, None], c64[:, 1, None, None]
    I = s64[:, 1, None, None]
    D = (s64[:, 2] + s64[:, 3] + _f32c(eps))[:, None, None]
    F = (2 * t * D - 2 * I) / (D * D)
    eF = (8 * EPS32 + DIV_ULPS * ULP32) * ((2 * t * D).abs() + (2 * I).abs()) / (D * D)
    dz = cb * (p - t) + cd * (p * (1 - p)) * F
    edz = cb.abs() * (r["ep"] + EPS32 * (p - t).abs()) + \
        cd.abs() * (r["ep"] * F.abs() + p * (1 - p) * (eF + 4 * EPS32 * F.abs())) + 2 * EPS32 * dz.abs()
    ref = W.t() @ dz @ W
    cnt = (W > 0).sum(0).double()
    adz = W.t() @ dz.abs() @ W
    bound = W.t() @ edz @ W + r["cs"] * (Dm.t() @ dz.abs() @ W + W.t() @ dz.abs() @ Dm) + \
        (cnt[:, None] + cnt[None, :] + 8) * EPS32 * adz + EPS32 * ref.abs()
    return ref, bound


def seg_loss_emulate(lr, tgt, sums, coef, eps, bwd_tgt=None, swap_wy=False):
    """Both kernels' per-pixel arithmetic in torch fp32 (gathers and lerps as the kernel orders them); the sums in plain
    fp32 torch reductions.  Returns partial [B, chunks, 4] and dlogits_lr [B, g, g].
    Mutants for the host test: bwd_tgt replaces the mask the BACKWARD reads (a transposed or shifted one: a wrong index
    into the targets), swap_wy exchanges wy and 1 - wy in the backward's row gather."""
    g, S = lr.shape[-1], tgt.shape[-1]
    f = torch.float32
    scale = torch.tensor(float(g), dtype=f) / torch.tensor(float(S), dtype=f)
    i = torch.arange(S, dtype=f)
    s = (scale * (i + 0.5) - 0.5).clamp_min(0.0)
    i0 = s.floor().clamp_max(g - 1).long()
    i1 = (i0 + 1).clamp_max(g - 1)
    w = s - i0.to(f)
    L, t = lr.float(), tgt.float()
    wx, wy = w[None, None, :], w[None, :, None]
    top = L[:, i0][:, :, i0] * (1 - wx) + L[:, i0][:, :, i1] * wx
    bot = L[:, i1][:, :, i0] * (1 - wx) + L[:, i1][:, :, i1] * wx
    z = top * (1 - wy) + bot * wy
    e = torch.exp2(-z.abs() * torch.tensor(LOG2E, dtype=f))
    bce = z.clamp_min(0) - z * t + torch.log1p(e)
    p = torch.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    chunks = (S + 7) // 8
    terms = torch.stack([bce, p * t, p, t], -1)
    part = torch.stack([terms[:, 8 * c:8 * c + 8].sum((1, 2)) for c in range(chunks)], 1)
    cb, cd = coef.float()[:, 0, None, None], coef.float()[:, 1, None, None]
    I = sums.float()[:, 1, None, None]
    D = (sums.float()[:, 2] + sums.float()[:, 3] + torch.tensor(eps, dtype=f))[:, None, None]
    invD2 = 1.0 / (D * D)
    tb = t if bwd_tgt is None else bwd_tgt.float()
    dz = cb * (p - tb) + cd * (p * (1 - p)) * ((2 * tb * D - 2 * I) * invD2)
    Wm = torch.zeros(S, g, dtype=f)
    r = torch.arange(S)
    Wm[r, i0] += 1 - w
    Wm[r, i1] += w
    Wy = Wm
    if swap_wy:
        Wy = torch.zeros(S, g, dtype=f)
        Wy[r, i0] += w
        Wy[r, i1] += 1 - w
    return part, Wy.t() @ dz @ Wm


# ---- AdamW -----------------------------------------------------------------------------------------------------
ADAMW_C = 2.0


def adamw_ref(p, g, m, v, lr, wd, beta1, beta2, eps, step, coef=None):
    """One torch.optim.AdamW step in float64 from the fp32 p, g, m, v (and the fp32 clip coefficient), and per-element
    bounds for the fp32 kernel, which rounds every product and sum once (contraction off) and every scalar from double:
      g' = g coef                            2^-24 |g'|
      m' = m + (g' - m)(1 - b1)              2^-24 (|m'| + 4 (1 - b1)(|g'| + |m|))
      v' = v b2 + g'^2 (1 - b2)              2^-24 (|v'| + 2 v b2 + 5 g'^2 (1 - b2))
      den = sqrt(v') / sqrt(bc2) + eps       the error of v' through the square root, min(sqrt(err), err / (2 sqrt(v')))
                                             (the second form alone is infinite at v' = 0), + (3 + SQRT_ULPS) 2^-24-ish
      p' = p (1 - lr wd) - (lr / bc1) m'/den 3 * 2^-24 |p| + |upd| (err(m') / |m'| + err(den) / den + (3 + DIV_ULPS 2) 2^-24)
                                             + 2^-24 |p'|.
    The counts above are the roundings of the code, and the fp32 emulation (the kernel's order in torch fp32, the same
    numbers torch's own fp32 AdamW gives) reaches 0.74 of them for exp_avg, 0.69 for exp_avg_sq, 0.58 for p: three
    roundings on terms of equal size leave no headroom.  By the file's convention the whole bound carries ADAMW_C = 2, which
    puts the measured worst at 0.37 (asserted <= 0.5 in tests/test_kernel_ref_host.py).
    Returns (p', bound), (m', bound), (v', bound)."""
    p64, g64, m64, v64 = p.double(), g.double(), m.double(), v.double()
    lr, wd = _f32c(lr), _f32c(wd)
    gs = g64 * (1.0 if coef is None else float(coef))
    m2 = m64 + (gs - m64) * (1 - beta1)
    v2 = v64 * beta2 + gs * gs * (1 - beta2)
    bc1, bc2 = 1 - beta1 ** step, 1 - beta2 ** step
    root = torch.sqrt(v2)
    den = root / math.sqrt(bc2) + eps
    upd = (lr / bc1) * (m2 / den)
    p2 = p64 * (1 - lr * wd) - upd
    em = EPS32 * (m2.abs() + 4 * (1 - beta1) * (gs.abs() + m64.abs()))
    ev = EPS32 * (v2.abs() + 2 * v64 * beta2 + 5 * gs * gs * (1 - beta2)) + TINY[torch.float32]
    eroot = torch.minimum(torch.sqrt(ev), ev / (2 * root).clamp_min(1e-300)) + SQRT_ULPS * EPS32 * root
    eden = (eroot + 2 * EPS32 * root) / math.sqrt(bc2) + EPS32 * den + EPS32 * eps
    eupd = (lr / bc1) * (em / den + m2.abs() * eden / (den * den)) + (3 + 2 * DIV_ULPS) * EPS32 * upd.abs()
    ep = 3 * EPS32 * p64.abs() + eupd + EPS32 * p2.abs() + TINY[torch.float32]
    return (p2, ADAMW_C * ep), (m2, ADAMW_C * (em + TINY[torch.float32])), (v2, ADAMW_C * ev)


# ---- antialiased resize, MixUp, normalise, layouts -------------------------------------------------------------
def aa_axis(out_size, in_size):
    """The triangle filter of upsample_bilinear2d(antialias=True) along one axis, restated in float64:
    scale = in / out, support = max(scale, 1), centre = scale (i + 0.5), taps j in [trunc(centre - support + 0.5) clamped
    at 0, trunc(centre + support + 0.5) clamped at `in`), weight max(0, 1 - |(j - centre + 0.5) / support|) / total.
    Returns W [out, in] and A [out], the bound on sum_j |w_fp32 - w| of one output: the fp32 centre and tap offsets are
    off by delta = 2 * 2^-24 (centre + support) / support + 2 * 2^-24, each raw weight by as much (a tap the fp32 range
    gains or loses sits where the triangle is zero, so this holds for it too), the normalisation doubles it:
    A = 2 n delta / total + (n + 2) 2^-24 with n taps (the n + 2: their products and the division)."""
    scale = in_size / out_size
    support = max(scale, 1.0)
    i = torch.arange(out_size, dtype=torch.float64)
    centre = scale * (i + 0.5)
    lo = torch.trunc(centre - support + 0.5).clamp_min(0)
    hi = torch.trunc(centre + support + 0.5).clamp_max(in_size)
    j = torch.arange(in_size, dtype=torch.float64)[None, :]
    raw = (1.0 - ((j - centre[:, None] + 0.5) / support).abs()).clamp_min(0.0)
    raw = raw * ((j >= lo[:, None]) & (j < hi[:, None]))
    total = raw.sum(1)
    W = raw / total[:, None]
    n = hi - lo
    delta = 2 * EPS32 * (centre + support) / support + 2 * EPS32
    return W, 2 * n * delta / total + (n + 2) * EPS32


def resize_ref(src, src_u8, S):
    """src: uint8 (B, Hs, Ws, 3) or float32 (B, 3, Hs, Ws) in [0, 1] -> float64 (B, 3, S, S) and its bound.
    Hs == S and Ws == S is the kernel's copy shortcut: exact (the u8 scale fl(1 / 255) apart: two roundings).  Otherwise
    Wy X Wx^T: pixels lie in [0, 1], so the weights' errors enter as Ay + Ax, and the two fp32 tap sums as
    (ny + nx + 2) 2^-24 of a value <= 1, which A already counts."""
    x = src.permute(0, 3, 1, 2).double() / 255.0 if src_u8 else src.double()
    Hs, Ws = x.shape[-2:]
    base = 2 * EPS32 if src_u8 else 0.0
    if Hs == S and Ws == S:
        return x, torch.full_like(x, base) * x
    Wy, Ay = aa_axis(S, Hs)
    Wx, Ax = aa_axis(S, Ws)
    out = Wy @ x @ Wx.t()
    bound = (Ay[:, None] + Ax[None, :] + base).expand_as(out).clone()
    return out, bound


def normalise_ref(v, ev, mean, std, out_dt):
    """(v - mean) fl(1 / std): (err(v) + 2^-24 (|v| + |mean|)) / std + 2 * 2^-24 |out|, then the store."""
    mean, std = _f32c(mean), _f32c(std)
    out = (v - mean) / std
    return out, (ev + EPS32 * (v.abs() + abs(mean))) / abs(std) + (2 * EPS32 + UNIT[out_dt]) * out.abs() + TINY[out_dt]


def patch_major(x, bound, P, Kp):
    """(B, 3, S, S) -> [B g g, Kp], k = c P P + ky P + kx, g = S // P (trailing pixels dropped), pad columns 0 with
    bound 0: they must be exactly zero."""
    B, C, S, _ = x.shape
    g = S // P

    def one(t):
        t = t[:, :, :g * P, :g * P].reshape(B, C, g, P, g, P).permute(0, 2, 4, 1, 3, 5).reshape(B * g * g, C * P * P)
        out = torch.zeros(B * g * g, Kp, dtype=t.dtype)
        out[:, :C * P * P] = t
        return out
    return one(x), one(bound)


def preprocess_ref(src, src_u8, S, P, Kp, patch, mean, std, mix_index, lam, out_dt):
    v, ev = resize_ref(src, src_u8, S)
    if mix_index is not None:
        lam = _f32c(lam)
        idx = mix_index.long()
        a, b = lam * v, (1.0 - lam) * v[idx]
        ev = abs(lam) * ev + abs(1.0 - lam) * ev[idx] + 3 * EPS32 * (a.abs() + b.abs())
        v = a + b
    out, bound = normalise_ref(v, ev, mean, std, out_dt)
    return patch_major(out, bound, P, Kp) if patch else (out, bound)


# ---- augmentation ----------------------------------------------------------------------------------------------
AUG_FIELDS = ("flip", "cos", "sin", "brightness", "contrast", "saturation", "hue", "order")
HUE_LIP = 7.0                    # see aug_ref
HUE_EXCUSED_CAP = 0.01


def _grey64(x):
    return 0.299 * x[0] + 0.587 * x[1] + 0.114 * x[2]


def _hue64(x, shift):
    """The header's hue operator on float64 (3, S, S): RGB -> HSV, h = frac(h + shift), HSV -> RGB.  Also returns the
    excusable mask: the two largest or the two smallest channels closer than 1e-5, or 6 h within 1e-4 of an integer."""
    r, g, b = x[0], x[1], x[2]
    srt = x.sort(0).values
    mx, mn = srt[2], srt[0]
    cr = mx - mn
    eq = cr == 0
    crd = torch.where(eq, torch.ones_like(cr), cr)
    sat = cr / torch.where(eq, torch.ones_like(cr), mx)
    rc, gc, bc = (mx - r) / crd, (mx - g) / crd, (mx - b) / crd
    isr = mx == r
    isg = (mx == g) & ~isr
    isb = ~isr & ~(mx == g)
    h = (isr * (bc - gc) + isg * (2.0 + rc - bc) + isb * (4.0 + gc - rc)) / 6.0 + 1.0
    h = h - h.floor()
    h = h + shift
    h = h - h.floor()
    h6 = h * 6.0
    fi = h6.floor()
    f = h6 - fi
    i = fi.long() % 6
    v = mx
    p = (v * (1 - sat)).clamp(0, 1)
    q = (v * (1 - f * sat)).clamp(0, 1)
    t = (v * (1 - (1 - f) * sat)).clamp(0, 1)
    R = torch.stack([v, q, p, p, t, v])
    G = torch.stack([t, v, v, q, p, p])
    Bl = torch.stack([p, p, t, v, v, q])
    pick = lambda tab: tab.gather(0, i[None])[0]
    excused = ((srt[2] - srt[1]) < 1e-5) | ((srt[1] - srt[0]) < 1e-5) | ((h6 - h6.round()).abs() < 1e-4)
    return torch.stack([pick(R), pick(G), pick(Bl)]), excused


def aug_ref(src, src_u8, S, table, mean, std, out_dt):
    """float64 reference of sgl_op_preprocess_aug, restating the header: resize, flip out(y, x) = in(y, S - 1 - x),
    rotation about ((S - 1) / 2, (S - 1) / 2) (counter-clockwise positive, out(p) = in(M^-1 p) bilinear, zeros outside),
    the colour operators in table order with the grey mean taken at the contrast step, normalise.
    table: one dict per image with AUG_FIELDS (floats already rounded to fp32; order a list of four, order[0] < 0 = no
    colour).  Returns out (B, 3, S, S), its bound, grey_mean (B), its bound, and the hue-excused mask (B, S, S).
    Error carried per pixel (one number for the three channels, e):
      rotation    the fp32 source position is off by 4 * 2^-24 S per axis, a bilinear sample of values in [0, 1] moves by
                  at most that per axis (continuous across the floor and into the zero border): (8 S + 8) 2^-24, plus the
                  taps' own e interpolated;
      brightness  |f| e + 2^-24;   contrast  |f| e + |1 - f| err(mean) + 4 (1 + |f|) 2^-24;
      saturation  (|f| + |1 - f|) e + (4 + 3 |1 - f|)(1 + |f|) 2^-24   (grey is a convex combination: e + 3 * 2^-24);
      hue         HUE_LIP e + 48 * 2^-24.  Within a sector the outputs are v, min, v - f cr, min + f cr with
                  f cr = (a - b) + c cr for two input channels a, b and a constant -1 < c < 2: linear in the inputs with
                  |coefficients| summing to at most 1 + 2 + 2 * 2 = 7, and continuous from sector to sector; the fp32
                  evaluation (differences of channels in [0, 1], divisions by cr that cancel again in f cr, h <= 2)
                  is within 48 roundings of a value <= 1;
      grey mean   mean(e + 3 * 2^-24) + (ceil(S S / 256) + BLOCK_TREE + 2) 2^-24 mean(grey)."""
    x, ex = resize_ref(src, src_u8, S)
    B = x.shape[0]
    ex = ex.amax(1)                                        # (B, S, S)
    outs, bounds, gms, gbs, masks = [], [], [], [], []
    ar = torch.arange(S, dtype=torch.float64)
    for b in range(B):
        a = table[b]
        im, e = x[b], ex[b]
        if a["flip"] != 0:
            im, e = im.flip(-1), e.flip(-1)
        if not (a["cos"] == 1.0 and a["sin"] == 0.0):
            ctr = 0.5 * (S - 1)
            dx, dy = ar[None, :] - ctr, ar[:, None] - ctr
            xs = a["cos"] * dx - a["sin"] * dy + ctr
            ys = a["sin"] * dx + a["cos"] * dy + ctr
            x0, y0 = xs.floor(), ys.floor()
            fx, fy = xs - x0, ys - y0
            nim, ne = torch.zeros_like(im), torch.zeros_like(e)
            for jy in (0, 1):
                for jx in (0, 1):
                    yy, xx = (y0 + jy).long(), (x0 + jx).long()
                    w = (fy if jy else 1 - fy) * (fx if jx else 1 - fx)
                    w = torch.where((yy >= 0) & (yy < S) & (xx >= 0) & (xx < S), w, torch.zeros_like(w))
                    yc, xc = yy.clamp(0, S - 1), xx.clamp(0, S - 1)
                    nim = nim + w * im[:, yc, xc]
                    ne = ne + w * e[yc, xc]
            im, e = nim, ne + (8 * S + 8) * EPS32
        gm, gb = torch.zeros((), dtype=torch.float64), torch.zeros((), dtype=torch.float64)
        mask = torch.zeros(S, S, dtype=torch.bool)
        order = a["order"]
        if order[0] >= 0:
            for op in order:
                if op == 0:
                    f = a["brightness"]
                    im, e = (im * f).clamp(0, 1), abs(f) * e + EPS32
                elif op == 1:
                    f = a["contrast"]
                    grey = _grey64(im)
                    gm = grey.mean()
                    gb = (e + 3 * EPS32).mean() + (math.ceil(S * S / 256) + BLOCK_TREE + 2) * EPS32 * gm
                    im, e = ((im - gm) * f + gm).clamp(0, 1), abs(f) * e + abs(1 - f) * gb + 4 * (1 + abs(f)) * EPS32
                elif op == 2:
                    f = a["saturation"]
                    grey = _grey64(im)
                    im = ((im - grey) * f + grey).clamp(0, 1)
                    e = (abs(f) + abs(1 - f)) * e + (4 + 3 * abs(1 - f)) * (1 + abs(f)) * EPS32
                else:
                    im, ex_b = _hue64(im, a["hue"])
                    mask |= ex_b
                    e = HUE_LIP * e + 48 * EPS32
        o, bo = normalise_ref(im, e[None].expand_as(im), mean, std, out_dt)
        outs.append(o), bounds.append(bo), gms.append(gm), gbs.append(gb), masks.append(mask)
    return torch.stack(outs), torch.stack(bounds), torch.stack(gms), torch.stack(gbs), torch.stack(masks)


# ---- seeded inputs shared by tests/test_kernel_ref_host.py and tests/test_kernel_edges_aux_gpu.py ----------------
def image_source(B, Hs, Ws, u8, seed):
    """A seeded source batch: uint8 (B, Hs, Ws, 3) or float32 (B, 3, Hs, Ws) in [0, 1].  A smooth colour ramp per image plus
    noise; the three channels of a uint8 pixel are made distinct (a pixel with two equal channels is one the hue rule may
    excuse, and one random byte triple in 85 has a pair: over the 1 % cap on an un-resized source)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    yy = torch.linspace(0, 1, Hs)[None, None, :, None]
    xx = torch.linspace(0, 1, Ws)[None, None, None, :]
    ph = torch.rand(B, 3, 1, 1, generator=g)
    img = 0.5 + 0.3 * torch.sin(6.0 * (yy * (1 + ph) + xx * (2 - ph)) + 6.28 * ph) + 0.2 * (torch.rand(B, 3, Hs, Ws, generator=g) - 0.5)
    img = img.clamp(0, 1)
    if not u8:
        return img.contiguous()
    q = (img * 255).round().to(torch.int64)
    q[:, 1] = torch.where(q[:, 1] == q[:, 0], (q[:, 1] + 7) % 256, q[:, 1])
    for _ in range(2):
        clash = (q[:, 2] == q[:, 0]) | (q[:, 2] == q[:, 1])
        q[:, 2] = torch.where(clash, (q[:, 2] + 13) % 256, q[:, 2])
    return q.permute(0, 2, 3, 1).to(torch.uint8).contiguous()


def aug_table():
    """One record per branch of the augmentation kernels (see tests/test_kernel_edges_aux_gpu.py); floats are rounded to
    fp32 here so the reference and the device table read the same numbers."""
    c5, s5 = math.cos(math.radians(5.0)), math.sin(math.radians(5.0))
    N = dict(flip=0.0, cos=1.0, sin=0.0, brightness=1.0, contrast=1.0, saturation=1.0, hue=0.0, order=[-1, 0, 0, 0])
    rec = lambda **kw: {**N, **kw}
    allf = dict(brightness=1.1, contrast=0.85, saturation=1.2, hue=0.04)
    tab = [
        rec(),                                                                    # no-op
        rec(flip=1.0),                                                            # flip only
        rec(cos=c5, sin=s5),                                                      # rotation only, +5 degrees
        rec(cos=c5, sin=-s5),                                                     # rotation only, -5 degrees
        rec(flip=1.0, brightness=1.1, order=[0, 1, 2, 3]),                        # (1, 0) shortcut; brightness alone
        rec(order=[1, 0, 2, 3], **allf),                                          # contrast first
        # contrast last, after flip + rotation.  No hue step here (saturation twice instead): the zero corners a rotation
        # leaves are 2 % of the image, every one a pixel the hue rule may excuse (three equal channels), which would
        # put this image over the per-image cap; hue after other operators is records 5 and 7, hue before contrast 11
        rec(flip=1.0, cos=c5, sin=s5, order=[0, 2, 2, 1], **allf),
        rec(order=[0, 2, 3, 0], brightness=0.9, saturation=0.7, hue=-0.03),       # contrast absent: grey_mean = 0
        rec(contrast=1.3, order=[0, 1, 2, 3]),                                    # contrast alone
        rec(saturation=0.6, order=[0, 1, 2, 3]),                                  # saturation alone
        rec(hue=0.05, order=[0, 1, 2, 3]),                                        # hue alone
        rec(flip=1.0, hue=-0.05, order=[3, 2, 1, 0]),                             # hue alone, negative, first
    ]
    for r in tab:
        for k in AUG_FIELDS[:-1]:
            r[k] = _f32c(r[k])
    return tab


# name, source is uint8, output dtype code, (Hs, Ws), S, P, Kp, patch-major
AUG_CASES = [
    ("u8_f32_nchw_s42", True, F32, (97, 131), 42, 14, 640, False),               # S*S no multiple of 256
    ("u8_bf16_patch_s14_pad", True, BF16, (30, 30), 14, 7, 192, True),           # S*S < 256; bf16 pad columns
    ("u8_f16_patch_s45_p14_pad", True, F16, (45, 45), 45, 14, 640, True),        # un-resized; S % P != 0; f16 pad
    ("f32_f32_patch_s45_p14_pad", False, F32, (50, 50), 45, 14, 640, True),      # S % P != 0; f32 pad columns
    ("f32_bf16_nchw_s42", False, BF16, (42, 42), 42, 14, 640, False),            # preprocess_aug_kernel<false, bf16>
    ("f32_f16_nchw_s42", False, F16, (64, 40), 42, 14, 640, False),
]


def aug_case_inputs(name):
    """(source, table) of one AUG_CASES entry: as many images as the table has records."""
    i = [c[0] for c in AUG_CASES].index(name)
    _, u8, _, (Hs, Ws), _, _, _, _ = AUG_CASES[i]
    tab = aug_table()
    return image_source(len(tab), Hs, Ws, u8, seed=500 + i), tab


def seg_inputs(B, g, S, seed):
    """Low-res logits [B, g, g] with part of the map scaled to +-30, targets [B, S, S] with image 0 all zero, image 1 all
    one, image 2 random with zero coefficients (dlogits_lr exactly 0) and image 3 random under a band of ones with non-zero
    coefficients (SEG_B = 4 images)."""
    gen_ = torch.Generator(device="cpu").manual_seed(seed)
    lr = torch.randn(B, g, g, generator=gen_) * 2.5
    lr[:, : max(1, g // 2), : max(1, g // 3)] *= 12.0
    lr = lr.clamp(-30, 30)
    tgt = (torch.rand(B, S, S, generator=gen_) < 0.3).float()
    tgt[0] = 0.0
    if B > 1:
        tgt[1] = 1.0
    if B > 3:                                            # image 3: a mask that is neither uniform nor symmetric, with
        tgt[3, : max(1, S // 3), :] = 1.0                # non-zero coefficients: a wrongly indexed mask read shows
    coef = torch.tensor([[1.7e-5, -0.21], [0.9e-5, -0.4], [0.0, 0.0], [2.0e-5, -0.3]])[:B].clone()
    return lr, tgt, coef


SEG_B = 4
SEG_CASES = [(1, 8), (4, 56), (3, 42), (27, 320), (16, 257), (14, 14), (27, 14)]
L2_SHAPES = [(1, 1, 1), (3, 4, 100), (2, 3, 257), (2, 32, 1152), (1, 1, 16380)]
L2_MAX_D = 16380


def l2_inputs(B, T, D, seed):
    """Frames of norm about 3 sqrt(D), with frame 0 scaled to norm 1e-18 and the last frame to 1e18 when there are at
    least three frames."""
    gen_ = torch.Generator(device="cpu").manual_seed(seed)
    f = torch.randn(B * T, D, generator=gen_) * 3
    if B * T >= 3:
        f[0] = f[0] / f[0].norm() * 1e-18
        f[-1] = f[-1] / f[-1].norm() * 1e18
    return f, torch.randn(B, D, generator=gen_)


# ===============================================================================================================
# kernels only the encoder calls (csrc/elementwise.hip, layernorm.hip; tests/test_kernel_edges_internal_gpu.py)
#
# Casts and splits are exact (bit-equal to torch's round-to-nearest).  Sums carry the fp32-accumulation bound of `sum_ref`,
# no constant.  The pooling-head attention bounds are derived term by term below; their one measured ingredient is the
# `__expf` term, evaluated on the test's own scores (`expf_eval_term`, the convention of `gelu_eval_term`).  One constant
# is fitted, by the convention at the top of this file:
#   POS_BWD_C = 32  pos_resize_bwd: the absolute error, in units of 2^-24, of one fp32 cubic weight beyond the share of the
#                 source coordinate's rounding (which is derived: resize_matrix_slack).  Measured on the axes of
#                 POS_BWD_GRIDS as max(|R32 - R64| - coordinate slack) / 2^-24 = 11.6 (axis 2 -> 5; 17.2 over all pairs
#                 of {2, 3, 14, 16, 24, 27, 37} x 1..39); 11.6 x 2.76 = 32.  With it the emulation's worst err/bound over
#                 POS_BWD_GRIDS (D = 5 and 144, three seeds, zero and normal priors) is 0.16; with c = 0 it is 1.85.
# ===============================================================================================================
POS_BWD_C = 32.0


def sum_ref(terms, prior=None, n=None):
    """ref = terms.sum(0) (+ prior) in float64; bound n u / (1 - n u) sum|terms| with n the number of addends (the prior
    of an accumulating kernel is one more): any order of n - 1 fp32 additions, and one more rounding for a product that
    was rounded before it was added (callers pass n accordingly)."""
    t = terms.double()
    ref, mag = t.sum(0), t.abs().sum(0)
    cnt = t.shape[0] if n is None else n
    if prior is not None:
        ref, mag, cnt = ref + prior.double(), mag + prior.double().abs(), cnt + 1
    g = cnt * EPS32 / (1 - cnt * EPS32)
    return ref, g * mag


def vecmat_ref(v, W, prior=None):
    """out[j] = sum_i v[i] W[i, j]: `rows` products (fused or not: n = rows + 1) in any order."""
    return sum_ref(v.double()[:, None] * W.double(), prior, n=W.shape[0] + 1)


def split3_ref(x):
    """hi = bf16(x), lo = bf16(x - hi): the subtraction is exact in fp32 (the rounding error of a narrower format is
    representable), so both are torch round-to-nearest conversions."""
    hi = x.float().to(torch.bfloat16)
    lo = (x.float() - hi.float()).to(torch.bfloat16)
    return hi, lo


def split3_layout(x, Cs, b_side, stacked):
    """The documented operand: rows [hi | hi | lo] / [hi | lo | hi] of Cs-wide segments, or the same three as planes."""
    R, C = x.shape
    hi, lo = (torch.zeros(R, Cs, dtype=torch.bfloat16, device=x.device) for _ in range(2))
    hi[:, :C], lo[:, :C] = split3_ref(x)
    seg = [hi, lo, hi] if b_side else [hi, hi, lo]
    return torch.cat(seg, 0) if stacked else torch.cat(seg, 1)


def split3_special_values():
    """+-0, fp32 subnormals, bf16 rounding ties (round to even both ways), values next to ties, the largest fp32 that does
    not round to a bf16 infinity, and its neighbours; then NaN and +-inf (hi keeps the class, lo = x - hi is NaN)."""
    bits = [0x00000000, 0x80000000, 0x00000001, 0x807FFFFF, 0x00400000, 0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF,
            0xBF818000, 0x7F7F7FFF, 0xFF7F7FFF, 0x7F7F0000, 0x7F7E8000, 0x00800000, 0x00808000, 0x3EAAAAAB, 0x4B7FFFFF,
            0x7FC00000, 0x7F800000, 0xFF800000]
    return torch.tensor(bits, dtype=torch.int64).to(torch.int32).view(torch.float32)


# ---- position-table resize, backward ---------------------------------------------------------------------------
def _cubic_w(t):
    A = -0.75
    x0, x1, x2, x3 = t + 1.0, t, 1.0 - t, 2.0 - t
    return torch.stack([((A * x0 - 5 * A) * x0 + 8 * A) * x0 - 4 * A, ((A + 2) * x1 - (A + 3)) * x1 * x1 + 1,
                        ((A + 2) * x2 - (A + 3)) * x2 * x2 + 1, ((A * x3 - 5 * A) * x3 + 8 * A) * x3 - 4 * A], -1)


def resize_matrix(n_in, n_out, dtype=torch.float64, shift=None, mask=False):
    """Dense [n_out, n_in] matrix of the one-axis bicubic resize (A = -0.75, align_corners=False, clamped taps) in
    `dtype`; in float32 every step is the kernel's (cubic_taps of csrc/elementwise.hip), clamped taps that meet on one
    border entry being added in tap order.  `shift` [n_out] moves the source coordinates (see resize_matrix_slack);
    mask=True returns which entries are taps instead."""
    o = torch.arange(n_out, dtype=dtype)
    scale = (torch.tensor(float(n_in), dtype=dtype) / torch.tensor(float(n_out), dtype=dtype))
    src = scale * (o + 0.5) - 0.5
    if shift is not None:
        src = src + shift
    fl = torch.floor(src)
    w = _cubic_w(src - fl)
    M = torch.zeros(n_out, n_in, dtype=dtype)
    for k in range(4):
        idx = (fl.long() - 1 + k).clamp(0, n_in - 1)
        M[torch.arange(n_out), idx] += 1.0 if mask else w[:, k]
    return M != 0 if mask else M


def resize_matrix_slack(n_in, n_out, c):
    """How far an entry of the fp32 resize matrix can be from the float64 one, entry by entry.
    Coordinate: scale = n_in / n_out, scale * (o + 0.5) and the - 0.5 are one rounding each of a number no larger than
    |src| + 0.5, so the coordinate is off by at most delta = 4 2^-24 (|src| + 1).  The matrix is a continuous function of
    the coordinate (the cubic convolution kernel is C1 and the clamp merges taps continuously), so over +-delta an entry
    moves by at most the larger of its two end-point changes (delta is 1e-5 at the most: an entry is monotone over it
    except within delta^2 of an extremum).  At g0 = 27 this reaches 120 2^-24 (a weight of 0.2 at coordinate 23.8 is off
    by 22 2^-24), and an integer coordinate (scale 5.4 at o = 2 gives 13.0) gets taps the float64 matrix does not have.
    Polynomials: Horner steps on coefficients up to 8 |A| = 6 leave an ABSOLUTE error of a few 2^-24 whatever the weight
    (5.2 2^-24 on the weight -0.024 of 27 -> 5): c 2^-24 on every tap, c = POS_BWD_C from the emulation."""
    o = torch.arange(n_out, dtype=torch.float64)
    src = (n_in / n_out) * (o + 0.5) - 0.5
    delta = 4 * EPS32 * (src.abs() + 1)
    R = resize_matrix(n_in, n_out)
    Rp, Rm = resize_matrix(n_in, n_out, shift=delta), resize_matrix(n_in, n_out, shift=-delta)
    taps = (resize_matrix(n_in, n_out, mask=True) | resize_matrix(n_in, n_out, shift=delta, mask=True)
            | resize_matrix(n_in, n_out, shift=-delta, mask=True))
    return torch.maximum((Rp - R).abs(), (Rm - R).abs()) + c * EPS32 * taps.double()


def pos_resize_bwd_ref(dout, g0, gh, gw, prior, c=POS_BWD_C):
    """dtable = prior + R^T dout with R = Ry (x) Rx dense in float64.  Bound per table element:
      terms 2^-24 (|Ry|^T |dout| |Rx| + |prior|)  +  ((|Ry| + Ey)^T |dout| (|Rx| + Ex) - |Ry|^T |dout| |Rx|)
    terms = one product and one addition for each output that touches the element (2 n_y n_x), the n_y row products and
    additions, the add into the table.  E = resize_matrix_slack(c): the fp32 evaluation of the weights, whose error is
    absolute in the weight (coordinate error times slope, polynomial cancellation), not relative to it.  The plain form
    (terms + c) 2^-24 sum|w||dout| does not describe that: the emulation would need c = 212 at grid (27, 1, 5), where
    weights of 0.02 to 0.2 carry 5 to 22 2^-24 each, and c would grow with g0 (tests/test_kernel_ref_host.py asserts it).
    Where the weights are of order 1 the two forms agree."""
    D = dout.shape[-1]
    Ry, Rx = resize_matrix(g0, gh), resize_matrix(g0, gw)
    G = dout.double().view(gh, gw, D)
    ref = torch.einsum("ya,yxd,xb->abd", Ry, G, Rx) + prior.double().view(g0, g0, D)
    mag = torch.einsum("ya,yxd,xb->abd", Ry.abs(), G.abs(), Rx.abs())
    Ey, Ex = resize_matrix_slack(g0, gh, c), resize_matrix_slack(g0, gw, c)
    weights = (torch.einsum("ya,yxd,xb->abd", Ry.abs() + Ey, G.abs(), Rx.abs() + Ex) - mag).clamp_min(0)
    ny, nx = (Ey != 0).sum(0).double(), (Ex != 0).sum(0).double()
    terms = (2 * ny[:, None] * nx[None, :] + 2 * ny[:, None] + 1)[:, :, None]
    bound = terms * EPS32 * (mag + prior.double().abs().view(g0, g0, D)) + weights
    return ref.reshape(g0 * g0, D), bound.reshape(g0 * g0, D)


def pos_resize_weight_excess(n_in, n_out):
    """max over entries of (|R32 - R64| - coordinate slack) / 2^-24: what POS_BWD_C has to cover (one axis)."""
    d = (resize_matrix(n_in, n_out, torch.float32).double() - resize_matrix(n_in, n_out)).abs()
    return ((d - resize_matrix_slack(n_in, n_out, 0.0)) / EPS32).max().item()


def pos_resize_bwd_emulate(dout, g0, gh, gw, prior):
    """pos_resize_bwd_kernel in torch fp32: fp32 weights, per table element the (oy, ox) order of the kernel, products and
    additions rounded separately (the kernel may fuse them: one rounding fewer)."""
    D = dout.shape[-1]
    Ry, Rx = resize_matrix(g0, gh, torch.float32), resize_matrix(g0, gw, torch.float32)
    G = dout.float().view(gh, gw, D)
    acc = torch.zeros(g0, g0, D)
    for oy in range(gh):
        row = torch.zeros(g0, D)
        for ox in range(gw):
            row = row + Rx[ox][:, None] * G[oy, ox][None, :]
        acc = acc + Ry[oy][:, None, None] * row[None]
    return (prior.float().view(g0, g0, D) + acc).view(g0 * g0, D)


POS_BWD_GRIDS = [(2, 3, 7), (3, 7, 3), (14, 16, 27), (27, 1, 5), (27, 16, 27), (14, 27, 16),   # test_posresize_rect's
                 (3, 3, 3), (2, 37, 5), (27, 1, 1)]                                           # identity, steep up, steep down


# ---- pooling-head attention (one query per head) ----------------------------------------------------------------
def pool_inputs(kind, B, H, N, dh, DP, tdt, seed=0):
    """q [H * dh] fp32 (a different query per head), K, V [B, H, N, DP] of `tdt` with zero pad columns, dout [B, H * dh].
    gauss: unit normals.  big: scores of magnitude about 60 and one dominant key per (image, head) at about +90 (the max
    subtraction).  equal: every key of a head the same vector (all-equal scores)."""
    g = torch.Generator().manual_seed(seed * 7919 + N * 31 + dh)
    rn = lambda *s: torch.randn(*s, generator=g)
    q = rn(H, dh)
    K, V = torch.zeros(B, H, N, DP), torch.zeros(B, H, N, DP)
    K[..., :dh], V[..., :dh] = rn(B, H, N, dh), rn(B, H, N, dh)
    if kind == "big":
        K[..., :dh] *= 20.0
        qn = q / (q * q).sum(-1, keepdim=True)
        for b in range(B):
            for h in range(H):
                K[b, h, (7 * b + 3 * h + N // 2) % N, :dh] = qn[h] * (90.0 * math.sqrt(dh))
    elif kind == "equal":
        K[..., :dh] = K[:, :, :1, :dh]
    else:
        assert kind == "gauss"
    return q.reshape(-1).contiguous(), K.to(tdt), V.to(tdt), rn(B, H * dh)


def expf_eval_term(x64):
    """4 x the largest relative deviation of the kernel's `__expf(x)` = exp2(x log2 e), evaluated in fp32 at the fp32
    rounding of the float64 arguments `x64` (so the rounding of the max subtraction is counted), from float64 exp, over
    the arguments above -80 (below, the result is under 2^-115 and the absolute floor of pool_attn_fwd_ref takes over).
    The hardware exp2 may be an ulp or two worse than libm: hence the 4."""
    x = x64.flatten()
    x = x[x > -80.0]
    if x.numel() == 0:
        return 4 * EPS32
    e32 = torch.exp2(x.float() * torch.tensor(LOG2E, dtype=torch.float32)).double()
    e64 = torch.exp(x)
    return max(4.0 * ((e32 - e64).abs() / e64).max().item(), 4 * EPS32)


POOL_FLOOR = 2.0 ** -120         # absolute floor of a probability (fp32 results below 2^-126 may be flushed)


def pool_attn_fwd_ref(q, K, V, H, dh, out_dt):
    """float64 softmax attention, one query per head: (probs [B, H, N], bound), (out [B, H * dh], bound).
    scores: a dh-term fp32 dot and the scale: eS_n = (dh + 2) 2^-24 scale sum|q||k_n|.  A score error moves every
    probability of the row by at most e^(2 max eS) - 1 relative.  Then `__expf` (expf_eval_term on these scores), the
    N-term sum of positive terms (N 2^-24 relative in any order), 1 / sum and the product (4 roundings):
      bound(p) = p (2 max_n eS_n + E_exp + (N + 4) 2^-24) + 2^-120.
    out_d = sum_n p_n V_nd with the kernel's own p: sum_n bound(p_n) |V_nd| + (N + 2) 2^-24 sum p |V| + u_out |out| + tiny."""
    B, _, N, DP = K.shape
    q64, K64, V64 = q.double().view(H, dh), K.double()[..., :dh], V.double()[..., :dh]
    scale = dh ** -0.5
    S = torch.einsum("hd,bhnd->bhn", q64, K64) * scale
    eS = (dh + 2) * EPS32 * scale * torch.einsum("hd,bhnd->bhn", q64.abs(), K64.abs())
    x = S - S.max(-1, keepdim=True).values
    Pr = torch.softmax(S, -1)
    rel = 2 * eS.max(-1, keepdim=True).values + expf_eval_term(x) + (N + 4) * EPS32
    bP = Pr * rel + POOL_FLOOR
    out = torch.einsum("bhn,bhnd->bhd", Pr, V64)
    bout = (torch.einsum("bhn,bhnd->bhd", bP, V64.abs()) + (N + 2) * EPS32 * torch.einsum("bhn,bhnd->bhd", Pr, V64.abs())
            + UNIT[out_dt] * out.abs() + TINY[out_dt])
    return (Pr, bP), (out.reshape(B, H * dh), bout.reshape(B, H * dh))


def pool_attn_bwd_ref(q, K, V, probs, dout, H, dh, out_dt):
    """float64 backward from the fp32 probabilities the kernel is given: (dkv [B * N, 2 H dh], bound), (dq [B, H dh], bound).
      dp_n = do . V_n                 e_dp_n = (dh + 1) 2^-24 sum|do||V_n|
      dot  = sum_n p_n dp_n           e_dot  = sum p_n e_dp_n + (N + 2) 2^-24 sum p_n |dp_n|
      ds_n = p_n (dp_n - dot) scale   e_ds_n = scale p_n (e_dp_n + e_dot + 3 2^-24 (|dp_n| + |dot|))
      dK_nd = ds_n q_d                e_ds_n |q_d| + (2^-24 + u_out) |dK| + tiny
      dV_nd = p_n do_d                (2^-24 + u_out) |dV| + tiny
      dq_d  = sum_n ds_n K_nd         sum_n e_ds_n |K_nd| + (N + 3) 2^-24 sum_n |ds_n K_nd|
    Each also carries the absolute floor 2^-120 times (1 + the magnitude of its other factor): a probability in fp32's
    subnormal range (the `big` family has them) has no relative precision, and the hardware may flush it."""
    B, _, N, DP = K.shape
    q64, K64, V64 = q.double().view(H, dh), K.double()[..., :dh], V.double()[..., :dh]
    P64, dO = probs.double().view(B, H, N), dout.double().view(B, H, dh)
    scale = dh ** -0.5
    dp = torch.einsum("bhd,bhnd->bhn", dO, V64)
    e_dp = (dh + 1) * EPS32 * torch.einsum("bhd,bhnd->bhn", dO.abs(), V64.abs())
    dot = (P64 * dp).sum(-1, keepdim=True)
    e_dot = (P64 * e_dp).sum(-1, keepdim=True) + (N + 2) * EPS32 * (P64 * dp.abs()).sum(-1, keepdim=True)
    ds = P64 * (dp - dot) * scale
    e_ds = scale * P64 * (e_dp + e_dot + 3 * EPS32 * (dp.abs() + dot.abs()))
    u, tiny = UNIT[out_dt], TINY[out_dt]
    dK = ds[..., None] * q64[None, :, None, :]
    bK = e_ds[..., None] * q64.abs()[None, :, None, :] + (EPS32 + u) * dK.abs() + tiny + POOL_FLOOR * (1 + q64.abs()[None, :, None, :])
    dV = P64[..., None] * dO[:, :, None, :]
    bV = (EPS32 + u) * dV.abs() + tiny + POOL_FLOOR * (1 + dO.abs()[:, :, None, :])
    tok = lambda t: t.permute(0, 2, 1, 3).reshape(B * N, H * dh)          # [B, H, N, dh] -> token-major [B N, H dh]
    dkv, bkv = torch.cat([tok(dK), tok(dV)], 1), torch.cat([tok(bK), tok(bV)], 1)
    dq = torch.einsum("bhn,bhnd->bhd", ds, K64)
    bq = (torch.einsum("bhn,bhnd->bhd", e_ds, K64.abs())
          + (N + 3) * EPS32 * torch.einsum("bhn,bhnd->bhd", ds.abs(), K64.abs())
          + POOL_FLOOR * (1 + K64.abs().sum(2)))
    return (dkv, bkv), (dq.reshape(B, H * dh), bq.reshape(B, H * dh))


def pool_attn_emulate(q, K, V, dout, H, dh, out_dt, probs=None):
    """pool_attn_fwd_kernel / pool_attn_bwd_kernel in torch fp32 (chunk partials of 8 columns, exp as exp2(x log2 e),
    plain fp32 sums in torch's order).  Returns probs, out and, when dout is given, dkv and dq from `probs` (the
    backward's input; default: its own)."""
    B, _, N, DP = K.shape
    f = torch.float32
    qf, Kf, Vf = q.float().view(H, dh), K.float()[..., :dh], V.float()[..., :dh]
    scale = torch.tensor(dh ** -0.5, dtype=f)
    part = (qf[None, :, None, :] * Kf).view(B, H, N, dh // 8, 8).sum(-1)
    S = part.sum(-1) * scale
    e = torch.exp2((S - S.max(-1, keepdim=True).values) * torch.tensor(LOG2E, dtype=f))
    Pr = e * (1.0 / e.sum(-1, keepdim=True))
    out = (Pr[..., None] * Vf).sum(2).reshape(B, H * dh).to(out_dt)
    if dout is None:
        return Pr, out
    Pb = Pr if probs is None else probs.float().view(B, H, N)
    dO = dout.float().view(B, H, dh)
    dp = (dO[:, :, None, :] * Vf).view(B, H, N, dh // 8, 8).sum(-1).sum(-1)
    dot = (Pb * dp).sum(-1, keepdim=True)
    ds = Pb * (dp - dot) * scale
    tok = lambda t: t.permute(0, 2, 1, 3).reshape(B * N, H * dh)
    dkv = torch.cat([tok(ds[..., None] * qf[None, :, None, :]), tok(Pb[..., None] * dO[:, :, None, :])], 1).to(out_dt)
    dq = (ds[..., None] * Kf).sum(2).reshape(B, H * dh)
    return Pr, out, dkv, dq
