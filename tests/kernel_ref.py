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
