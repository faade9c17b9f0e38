"""CPU tests of tests/kernel_ref.py: the bounds the GPU kernel tests assert are honest without a GPU.

For every bound: an fp32 emulation of the kernel's precision recipe stays inside it, a truncating one does not, and the
float64 reference agrees with torch autograd.  The constants that come from an emulation (LN_C, ATTN_BWD_K, the GELU
evaluation term) are re-measured here and asserted against the values kernel_ref.py states.
"""
import math

import pytest
import torch

import kernel_ref as kr

LO = [torch.bfloat16, torch.float16]


# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", [(300, 264, 1152), (257, 144, 4352), (64, 64, 8)])
@pytest.mark.parametrize("dt", LO, ids=["bf16", "f16"])
def test_gemm_bound_holds_for_fp32_matmul_and_catches_truncation(M, N, K, dt):
    """torch's own fp32 matmul stands in for the kernel: inside the bound with round-to-nearest (worst element measured
    at 0.15 to 0.99 of it), outside with a truncating store (1.08 to 1.97) wherever the output rounding is the larger
    part of the bound.  For fp16 at K = 4352 the accumulation term (K + 4) 2^-24 |A|.|B| is several times u |ref| and a
    truncating store stays inside (0.29): there the rounding-bias statistic is what catches it, so it is asserted for
    every case of at least 1e4 elements."""
    torch.manual_seed(M + N + K)
    A = torch.randn(M, K).to(dt)
    B = (torch.randn(N, K) / math.sqrt(K)).to(dt)
    bias = torch.randn(N)
    acc = A.float() @ B.float().t() + bias
    ref, bound, _ = kr.gemm_ref(A, B, K, kr.UNIT[dt], adds=(bias,))
    r = kr.assert_within(acc.to(dt), ref, bound, "fp32 matmul, rounded store")
    assert 0.1 < r <= 1.0
    if dt == torch.bfloat16 or K <= 1152:
        assert kr.worst_ratio(kr.truncate_to(acc, dt), ref, bound) > 1.05
        with pytest.raises(AssertionError):
            kr.assert_within(kr.truncate_to(acc, dt), ref, bound, "truncating store")
    if M * N >= 10000:
        assert abs(kr.rounding_bias(acc.to(dt), ref, kr.UNIT[dt])) < 0.03
        assert kr.rounding_bias(kr.truncate_to(acc, dt), ref, kr.UNIT[dt]) < -0.5


@pytest.mark.parametrize("dt", LO, ids=["bf16", "f16"])
def test_rounding_bias_separates_nearest_from_truncation(dt):
    torch.manual_seed(3)
    A = torch.randn(200, 192).to(dt)
    B = (torch.randn(136, 192) / math.sqrt(192)).to(dt)
    acc = A.float() @ B.float().t()
    ref = A.double() @ B.double().t()
    assert abs(kr.rounding_bias(acc.to(dt), ref, kr.UNIT[dt])) < 0.02
    assert kr.rounding_bias(kr.truncate_to(acc, dt), ref, kr.UNIT[dt]) < -0.5
    with pytest.raises(AssertionError):
        kr.assert_rounding_unbiased(kr.truncate_to(acc, dt), ref, kr.UNIT[dt], "truncating store")


def test_assert_within_excuses_nothing():
    ref = torch.ones(4, 5, dtype=torch.float64)
    bound = torch.full((4, 5), 1e-3, dtype=torch.float64)
    got = ref.clone()
    kr.assert_within(got, ref, bound, "exact")
    got[2, 3] += 2e-3                                     # one element out of twenty
    with pytest.raises(AssertionError, match=r"worst at \(2, 3\)"):
        kr.assert_within(got, ref, bound, "one bad element")
    got[2, 3] = float("nan")
    with pytest.raises(AssertionError):
        kr.assert_within(got, ref, bound, "NaN")


def test_gelu_formula_term_and_reference():
    """The fp32 x*sigmoid(2z) formula against float64 over N(0, 1.5) pre-activations: largest deviation 4.9e-7 (gelu: half
    an ulp of |x| < 8) and 1.9e-6 (derivative: the 1 - s cancellation times x (2z)' <= 35) measured, so the x 4 terms are
    1.9e-6 and 7.7e-6; asserted below 1e-5.  The float64 gelu and
    its derivative agree with torch."""
    torch.manual_seed(0)
    x = torch.randn(200000) * 1.5
    t, tg = kr.gelu_eval_term(x), kr.gelu_eval_term(x, grad=True)
    assert 0 < t < 1e-5 and 0 < tg < 1e-5, (t, tg)
    xd = x[:5000].double().requires_grad_(True)
    y = torch.nn.functional.gelu(xd, approximate="tanh")
    assert (kr.gelu64(xd) - y).abs().max().item() < 1e-14
    g, = torch.autograd.grad(y.sum(), xd)
    assert (kr.gelu_grad64(xd) - g).abs().max().item() < 1e-13


# ---------------------------------------------------------------------------------------------------------------
LN_DS = [4, 64, 516, 1152, 2048]


def _ln_measure(c):
    w = dict(y=0.0, mean=0.0, rstd=0.0, dx=0.0, dg=0.0, db=0.0)
    for seed in (0, 1, 2):
        for D in LN_DS:
            torch.manual_seed(D + seed)
            M = 64
            gam, bet = torch.randn(D) * 0.2 + 1, torch.randn(D) * 0.1
            for name, x in kr.ln_families(M, D, seed=D + 100 * seed).items():
                y, mu, rs = kr.ln_fwd_emulate(x, gam, bet, 1e-6, torch.float32)
                (yr, by), (mr, bm), (rr, br) = kr.ln_fwd_ref(x, gam, bet, 1e-6, kr.EPS32, c=c)
                dy, dres = torch.randn(M, D).bfloat16(), torch.randn(M, D)
                dx, _, dg, db = kr.ln_bwd_emulate(dy, x, mu, rs, gam, dres, torch.bfloat16)
                (dxr, b32, _), (dgr, bg), (dbr, bb) = kr.ln_bwd_ref(dy, x, mu, rs, gam, dres, kr.UNIT[torch.bfloat16],
                                                                    c=c)
                for k, v in dict(y=(y, yr, by), mean=(mu, mr, bm), rstd=(rs, rr, br), dx=(dx, dxr, b32),
                                 dg=(dg, dgr, bg), db=(db, dbr, bb)).items():
                    w[k] = max(w[k], kr.worst_ratio(*v))
    return w


def test_layernorm_constant_is_four_times_the_emulation():
    """LN_C = 28: with c = 1 the two-pass, wave-shaped fp32 emulation reaches 6.94 (y), 3.3 (mean), 4.3 (rstd), 1.9 (dx)
    of the bound over the input families (64 rows, D in {4, 64, 516, 1152, 2048}, three seeds); 4 x 6.94 = 27.8 <= 28 <=
    64.  dgamma / dbeta carry no constant."""
    w = _ln_measure(1.0)
    worst = max(w["y"], w["mean"], w["rstd"], w["dx"])
    assert 4 * worst <= kr.LN_C <= 64, w
    assert kr.LN_C <= 8 * worst, f"LN_C is more than twice the stated margin: {w}"
    assert w["dg"] <= 1 and w["db"] <= 1, w


@pytest.mark.parametrize("dt", LO, ids=["bf16", "f16"])
def test_layernorm_bounds_hold_and_catch_one_pass_variance_and_truncation(dt):
    torch.manual_seed(1)
    M, D = 16, 1152
    gam, bet = torch.randn(D) * 0.2 + 1, torch.randn(D) * 0.1
    for name, x in kr.ln_families(M, D, seed=5).items():
        y, mu, rs = kr.ln_fwd_emulate(x, gam, bet, 1e-6, dt)
        (yr, by), (mr, bm), (rr, br) = kr.ln_fwd_ref(x, gam, bet, 1e-6, kr.UNIT[dt])
        kr.assert_within(y, yr, by, f"{name} y")
        kr.assert_within(mu, mr, bm, f"{name} mean")
        kr.assert_within(rs, rr, br, f"{name} rstd")
    # a one-pass variance E[x^2] - mu^2 in fp32 loses everything at mean 1000, std 1: the bound must reject it
    x = kr.ln_families(M, D, seed=5)["mean1000"]
    mu1 = x.mean(-1)
    rs1 = 1.0 / torch.sqrt(((x * x).mean(-1) - mu1 * mu1).clamp_min(0) + 1e-6)
    (yr, by), _, (rr, br) = kr.ln_fwd_ref(x, gam, bet, 1e-6, kr.UNIT[dt])
    assert kr.worst_ratio(rs1, rr, br) > 10
    # a truncating 16-bit store is caught by the rounding-bias statistic and by the bound
    y32 = kr.ln_fwd_emulate(kr.ln_families(M, D, seed=5)["gauss"], gam, bet, 1e-6, torch.float32)[0]
    (yr, by), _, _ = kr.ln_fwd_ref(kr.ln_families(M, D, seed=5)["gauss"], gam, bet, 1e-6, kr.UNIT[dt])
    assert abs(kr.rounding_bias(y32.to(dt), yr, kr.UNIT[dt])) < 0.02
    assert kr.rounding_bias(kr.truncate_to(y32, dt), yr, kr.UNIT[dt]) < -0.5
    assert kr.worst_ratio(kr.truncate_to(y32, dt), yr, by) > 1


def test_layernorm_reference_matches_autograd():
    torch.manual_seed(2)
    M, D = 7, 64
    x = (torch.randn(M, D, dtype=torch.float64) * 2 + 0.3).requires_grad_(True)
    g = (torch.randn(D, dtype=torch.float64) * 0.2 + 1).requires_grad_(True)
    b = (torch.randn(D, dtype=torch.float64) * 0.1).requires_grad_(True)
    dy, dres = torch.randn(M, D, dtype=torch.float64), torch.randn(M, D, dtype=torch.float64)
    y = torch.nn.functional.layer_norm(x, (D,), g, b, 1e-6)
    gx, gg, gb = torch.autograd.grad(y, [x, g, b], dy)
    (yr, _), (mu, _), (rs, _) = kr.ln_fwd_ref(x.detach(), g.detach(), b.detach(), 1e-6, 0.0)
    assert (yr - y).abs().max().item() < 1e-12
    (dx, _, _), (dg, _), (db, _) = kr.ln_bwd_ref(dy, x.detach(), mu, rs, g.detach(), dres, 0.0)
    assert (dx - (gx + dres)).abs().max().item() < 1e-11
    assert (dg - gg).abs().max().item() < 1e-11 and (db - gb).abs().max().item() < 1e-11


# ---------------------------------------------------------------------------------------------------------------
def _attn_case(N, dh, sc, dt):
    q, k, v, do = kr.attn_inputs("gauss", 1, 1, N, dh, torch.float32, seed=N)
    q, k = (q * sc / 1.2).to(dt)[0, 0], (k * sc / 1.2).to(dt)[0, 0]
    return q, k, v.to(dt)[0, 0], do.to(dt)[0, 0]


@pytest.mark.parametrize("dt", LO, ids=["bf16", "f16"])
def test_attention_emulation_within_bounds_and_backward_constant(dt):
    """The recipe emulation (64-key online softmax, P and dS rounded, fp32 accumulate, delta from the rounded output) at
    N x dh of 729x72, 130x32, 300x64, 65x96, 1024x40 and input scales 0.05, 1.2, 4, 8.  Forward: at most 0.56 of the
    bound measured; lse at most 0.51 of 2^-20 (1 + |lse|).  Backward with k = 1: at most 0.86 (bf16) / 0.52 (fp16), so
    ATTN_BWD_K = 2 >= 2 x 0.86 and <= 8."""
    u = kr.UNIT[dt]
    worst_f = worst_l = worst_b = 0.0
    for (N, dh) in kr.ATTN_EMU_SHAPES:
        for sc in (0.05, 1.2, 4.0, 8.0):
            q, k, v, do = _attn_case(N, dh, sc, dt)
            O, lse, dQ, dK, dV = kr.attn_emulate(q, k, v, do, dt)
            r = kr.attn_ref(q, k, v, do)
            bO, bl = kr.attn_fwd_bound(r, u)
            worst_f = max(worst_f, kr.assert_within(O, r["O"], bO, f"O {N}x{dh} x{sc}"))
            worst_l = max(worst_l, kr.assert_within(lse, r["lse"], bl, f"lse {N}x{dh} x{sc}"))
            bQ, bK, bV = kr.attn_bwd_bound(r, u, k=1.0, tiny=kr.TINY[dt])
            for name, got, ref, bnd in (("dQ", dQ, r["dQ"], bQ), ("dK", dK, r["dK"], bK), ("dV", dV, r["dV"], bV)):
                worst_b = max(worst_b, kr.worst_ratio(got, ref, bnd))
    assert worst_f <= 0.7 and worst_l <= 0.7, (worst_f, worst_l)
    assert 2 * worst_b <= kr.ATTN_BWD_K <= 8, worst_b


@pytest.mark.parametrize("dt", LO, ids=["bf16", "f16"])
def test_attention_rounding_bias_catches_truncation(dt):
    """The element-wise attention bound is 3u |O| at its tightest, so it cannot see a P (or output) pack that truncates
    (error < 2u |O|).  With v, dout > 0 nothing cancels in P.V and P^T.dO, and the signed statistic
    mean((got - ref) / (u ref)) separates the two: round-to-nearest measures within +-0.01 on O and dV over 19200 elements,
    truncation below -0.7.  The GPU module asserts +-0.05, the same margin as for the GEMM store."""
    q, k, v, do = (t[0, 0] for t in kr.attn_inputs("positive", 1, 1, 300, 64, dt, seed=9))
    r = kr.attn_ref(q, k, v, do)
    O, _, _, _, dV = kr.attn_emulate(q, k, v, do, dt)
    assert abs(kr.rounding_bias(O, r["O"], kr.UNIT[dt])) < 0.02
    assert abs(kr.rounding_bias(dV, r["dV"], kr.UNIT[dt])) < 0.02
    O, _, _, _, dV = kr.attn_emulate(q, k, v, do, dt, rnd=lambda x: kr.truncate_to(x, dt))
    assert kr.rounding_bias(O, r["O"], kr.UNIT[dt]) < -0.5
    assert kr.rounding_bias(dV, r["dV"], kr.UNIT[dt]) < -0.5


@pytest.mark.parametrize("kind,jump", [("gauss", None), ("jump", 290), ("jump", 250), ("jump", 100), ("peaked", None),
                                       ("flat", None), ("offset", None)])
@pytest.mark.parametrize("dt", LO, ids=["bf16", "f16"])
def test_attention_hostile_inputs_stay_within_bounds_in_emulation(kind, jump, dt):
    """The input families of the GPU module through the emulation: the bounds hold for a correct recipe on each of them
    (so a GPU failure there is the kernel's), and every input stays inside fp16 range."""
    q, k, v, do = (t[0, 0] for t in kr.attn_inputs(kind, 1, 1, 300, 64, dt, seed=4, jump_key=jump))
    assert all(torch.isfinite(t.float()).all() for t in (q, k, v, do))
    O, lse, dQ, dK, dV = kr.attn_emulate(q, k, v, do, dt)
    r = kr.attn_ref(q, k, v, do)
    bO, bl = kr.attn_fwd_bound(r, kr.UNIT[dt])
    kr.assert_within(O, r["O"], bO, "O")
    kr.assert_within(lse, r["lse"], bl, "lse")
    bQ, bK, bV = kr.attn_bwd_bound(r, kr.UNIT[dt], tiny=kr.TINY[dt])
    kr.assert_within(dQ, r["dQ"], bQ, "dQ")
    kr.assert_within(dK, r["dK"], bK, "dK")
    kr.assert_within(dV, r["dV"], bV, "dV")
    if kind == "peaked":
        assert (r["P"].max(-1).values > 1 - 2.0 ** -24).float().mean().item() > 0.8, "softmax rows should be one-hot"
    if kind == "jump":
        assert r["P"][min(7, 299), jump].item() > 0.999


def test_attention_reference_matches_autograd():
    torch.manual_seed(5)
    q, k, v, do = (torch.randn(2, 3, 17, 8, dtype=torch.float64) for _ in range(4))
    qa, ka, va = (t.clone().requires_grad_(True) for t in (q, k, v))
    s = (qa @ ka.transpose(-1, -2)) * 8 ** -0.5
    o = torch.softmax(s, -1) @ va
    gq, gk, gv = torch.autograd.grad(o, [qa, ka, va], do)
    r = kr.attn_ref(q, k, v, do)
    assert (r["O"] - o).abs().max().item() < 1e-13
    assert (r["lse"] - torch.logsumexp(s, -1)).abs().max().item() < 1e-13
    for a, b in ((r["dQ"], gq), (r["dK"], gk), (r["dV"], gv)):
        assert (a - b).abs().max().item() < 1e-12


def test_colsum_and_pos_resize_references():
    torch.manual_seed(6)
    x = torch.randn(1000, 136)
    s = torch.zeros(136)
    for m in range(1000):
        s = s + x[m]
    ref, bound = kr.colsum_ref(x, 1000)
    kr.assert_within(s, ref, bound, "sequential fp32 column sum")
    t = torch.randn(9, 8)
    same = kr.pos_resize_ref(t, 3, 3, 3)
    assert (same - t.double()).abs().max().item() < 1e-12          # identity at the native size
    assert kr.pos_resize_ref(t, 3, 5, 2).shape == (10, 8)


# ===============================================================================================================
# kernels outside the encoder: every float64 reference against torch's own operator, every bound against an fp32
# emulation of the kernel at worst ratio <= 0.5 (the measured worst ratios are in the docstrings), and the hue cap.
# ===============================================================================================================
F = torch.nn.functional
HALF = 0.5


def _sums_of(part):
    return part.double().sum(1).float()


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_gate_mul_bound_grows_with_gate_and_holds_for_emulation(dt):
    """Measured worst emulation/bound: 0.43 (y), 0.46 (dg), 0.40 (dx) in fp32 over the sweep and N(0, 4) gates; 0.99 for
    bf16, whose store alone reaches its own half-ulp term.  The sigmoid bound at
    |g| = 80 is more than 20 times the one at 0 relative to (1 - s) s: the exponent's rounding, not a flat constant.
    A kernel that returned 1 - s for negative gates is far outside."""
    torch.manual_seed(0)
    n = 4096
    g = torch.randn(n) * 4
    g[: len(kr.GATE_SWEEP)] = torch.tensor(kr.GATE_SWEEP)
    g, x, dy = g.to(dt), torch.randn(n).to(dt), torch.randn(n).to(dt)
    y, dg, dx = kr.gate_mul_emulate(g, x, dy, dt)
    ref, b = kr.gate_mul_ref(g, x, dt)
    (rdg, bdg), (rdx, bdx) = kr.gate_mul_bwd_ref(dy, g, x, dt)
    worst = max(kr.assert_within(y, ref, b, "y"), kr.assert_within(dg, rdg, bdg, "dg"), kr.assert_within(dx, rdx, bdx, "dx"))
    # a bf16 store alone reaches its own term UNIT |y| (round-to-nearest is off by up to half an ulp = UNIT), so only the
    # fp32 case, where the derived terms are the whole bound, is held to one half
    assert worst <= (HALF if dt == torch.float32 else 1.0), worst
    gr, xr = g.double().requires_grad_(True), x.double().requires_grad_(True)
    (torch.sigmoid(gr) * xr).backward(dy.double())
    assert (gr.grad - rdg).abs().max() < 1e-12 and (xr.grad - rdx).abs().max() < 1e-12
    z = torch.tensor([0.0, -80.0])
    s, es = kr.sigmoid_fast_ref(z)
    rel = es / (s * (1 - s))
    assert rel[1] > 20 * rel[0]
    wrong = torch.where(g.float() < 0, 1 - torch.sigmoid(g.float()), torch.sigmoid(g.float())) * x.float()
    assert kr.worst_ratio(wrong.to(dt), ref, b) > 100


@pytest.mark.parametrize("flip", [0, 1])
def test_dwconv_reference_is_conv2d_and_bound_holds(flip):
    """Forward against nn.Conv2d(groups=E) in float64, flipped against its input gradient, the weight gradient against
    autograd; an fp32 conv inside the bound at 0.24 (forward) and 0.01 (weight gradient) measured."""
    torch.manual_seed(1 + flip)
    B, gh, gw, E = 2, 5, 7, 8
    x, dy = torch.randn(B, gh, gw, E), torch.randn(B, gh, gw, E)
    w9, bias = torch.randn(9, E), torch.randn(E)
    conv = torch.nn.Conv2d(E, E, 3, padding=1, groups=E).double()
    with torch.no_grad():
        conv.weight.copy_(w9.double().t().reshape(E, 1, 3, 3))
        conv.bias.copy_(bias.double())
    xin = x.double().permute(0, 3, 1, 2).requires_grad_(True)
    y = conv(xin)
    y.backward(dy.double().permute(0, 3, 1, 2))
    if flip:
        ref, b = kr.dwconv_ref(dy, w9, None, 1, torch.float32)
        assert (ref - xin.grad.permute(0, 2, 3, 1)).abs().max() < 1e-12
        got = F.conv2d(dy.permute(0, 3, 1, 2), w9.t().reshape(E, 1, 3, 3).flip(-1, -2), None, padding=1, groups=E)
    else:
        ref, b = kr.dwconv_ref(x, w9, bias, 0, torch.float32)
        assert (ref - y.permute(0, 2, 3, 1)).abs().max() < 1e-12
        got = F.conv2d(x.permute(0, 3, 1, 2), w9.t().reshape(E, 1, 3, 3), bias, padding=1, groups=E)
    assert kr.assert_within(got.permute(0, 2, 3, 1), ref, b, "fp32 conv") <= HALF
    prior = torch.randn(10, E)
    wref, wb = kr.dwconv_wgrad_ref(x, dy, prior)
    want = torch.cat([conv.weight.grad.reshape(E, 9).t(), conv.bias.grad[None]]) + prior.double()
    assert (wref - want).abs().max() < 1e-11
    emu = torch.stack([(kr._shift(x, k // 3, k % 3) * dy).reshape(-1, E).sum(0) for k in range(9)] +
                      [dy.reshape(-1, E).sum(0)]) + prior
    assert kr.assert_within(emu, wref, wb, "fp32 weight gradient") <= HALF


@pytest.mark.parametrize("B,T,D", kr.L2_SHAPES, ids=str)
def test_l2norm_tmean_reference_and_bound(B, T, D):
    """Against autograd of f / |f| -> mean in float64 and against the fp32 emulation (lane-shaped sums), rows of norm
    1e-18 and 1e18 included: worst ratio measured 0.13 for out, 0.13 for inv_norm, 0.18 for df."""
    f, g = kr.l2_inputs(B, T, D, seed=B * 10 + T)
    (out, bo), (inv, bi) = kr.l2norm_tmean_fwd_ref(f, B, T)
    fr = f.double().requires_grad_(True)
    o2 = (fr / fr.norm(dim=-1, keepdim=True)).view(B, T, D).mean(1)
    o2.backward(g.double())
    assert (o2 - out).abs().max() < 1e-14
    eo, einv, edf = kr.l2norm_emulate(f, g, B, T)
    df64, _ = kr.l2norm_tmean_bwd_ref(f, inv, g, B, T)                  # with the float64 inv_norm: autograd's own
    assert ((fr.grad - df64).abs() <= 1e-9 * (df64.abs() + g.double().abs().repeat_interleave(T, 0) * inv[:, None] / T)).all()
    df, bdf = kr.l2norm_tmean_bwd_ref(f, einv, g, B, T)                 # with the fp32 one the kernel is handed
    worst = max(kr.assert_within(eo, out, bo, "out"), kr.assert_within(einv, inv, bi, "inv_norm"),
                kr.assert_within(edf, df, bdf, "df"))
    assert worst <= HALF, worst


@pytest.mark.parametrize("g,S", kr.SEG_CASES, ids=str)
def test_seg_loss_reference_is_interpolate_bce_dice_and_bound_holds(g, S):
    """The partial sums against F.interpolate(bilinear) + BCE-with-logits / Dice terms in float64, dlogits_lr against
    autograd of sum_b c_bce sum(bce) + c_dice 2 I / D, and the fp32 emulation against both bounds: worst ratio measured
    0.07 (partials), 0.16 (dlogits_lr)."""
    B, eps = kr.SEG_B, 1e-6
    lr, tgt, coef = kr.seg_inputs(B, g, S, seed=g * 1000 + S)
    ref, bound = kr.seg_loss_fwd_ref(lr, tgt)
    L = lr.double().requires_grad_(True)
    up = F.interpolate(L[:, None], size=(S, S), mode="bilinear", align_corners=False)[:, 0]
    t = tgt.double()
    bce = F.binary_cross_entropy_with_logits(up, t, reduction="none")
    p = torch.sigmoid(up)
    want = torch.stack([bce.sum((1, 2)), (p * t).sum((1, 2)), p.sum((1, 2)), t.sum((1, 2))], -1)
    # the reference places its taps with the kernel's fp32 scale fl(g) / fl(S), torch with the double: positions differ by
    # 2^-24 g, values by that times a slope of up to 60
    assert ((ref.sum(1) - want).abs() <= 1e-4 * want.abs() + 1e-6).all()
    sums = _sums_of(ref)
    c = coef.double()
    s64 = sums.double()
    D = s64[:, 2] + s64[:, 3] + kr._f32c(eps)
    # d/dz of c_bce sum(bce) + c_dice 2 I / D with I, D as the kernel is handed them (constants of the fp32 sums)
    dz = c[:, 0, None, None] * (p - t) + c[:, 1, None, None] * p * (1 - p) * \
        ((2 * t * D[:, None, None] - 2 * s64[:, 1, None, None]) / (D * D)[:, None, None])
    up.backward(dz.detach())
    dref, dbound = kr.seg_loss_bwd_ref(lr, tgt, sums, coef, eps)
    assert ((dref - L.grad).abs() <= 1e-4 * L.grad.abs() + 1e-5 * L.grad.abs().max()).all()
    assert bool((dref[2] == 0).all()) and bool((dbound[2] == 0).all())       # zero coefficient rows: exact zeros
    part, dlr = kr.seg_loss_emulate(lr, tgt, sums, coef, eps)
    worst = max(kr.assert_within(part, ref, bound, "partials"), kr.assert_within(dlr, dref, dbound, "dlogits_lr"))
    assert worst <= HALF, worst
    # the mutant p -> 1 - p for z < 0 moves sum p out of its bound
    r = kr.seg_pixels_ref(lr, tgt)
    pm = torch.where(r["z"] < 0, 1 - r["p"], r["p"])
    assert ((pm.sum((1, 2))[:, None] - ref[..., 2].sum(1)[:, None]).abs() > bound[..., 2].sum(1)[:, None]).any()
    # backward mutants, seen through image 3 (a non-uniform, non-symmetric mask with non-zero coefficients): a mask read
    # at the transposed or at a shifted index, and wy <-> 1 - wy in the row gather.  With one low-res logit (g = 1) every
    # pixel feeds the same output with weight 1, so neither the order of the mask nor the weights can show.
    if g > 1:
        for name, kw in (("transposed mask", dict(bwd_tgt=tgt.transpose(1, 2))),
                         ("mask shifted by one row", dict(bwd_tgt=torch.roll(tgt, 1, dims=1))),
                         ("wy swapped", dict(swap_wy=True))):
            _, bad = kr.seg_loss_emulate(lr, tgt, sums, coef, eps, **kw)
            assert kr.worst_ratio(bad[3], dref[3], dbound[3]) > 10, name


@pytest.mark.parametrize("step,clip", [(1, None), (1000, 0.37), (1, 0.37), (1000, None)])
def test_adamw_reference_is_torch_adamw_and_bound_holds(step, clip):
    """One step against torch.optim.AdamW in float64 (state planted so that `step` is the bias-correction exponent), and
    torch's fp32 AdamW as the emulation (bit-identical to the kernel's order written out in torch fp32): worst ratio
    measured 0.29 (p), 0.37 (exp_avg), 0.34 (exp_avg_sq) with ADAMW_C = 2."""
    torch.manual_seed(step)
    n, lr, wd, b1, b2, eps = 5000, 3e-3, 0.05, 0.9, 0.999, 1e-8
    p, g = torch.randn(n), torch.randn(n) * 0.01
    m, v = torch.randn(n) * 0.01, torch.rand(n) * 1e-4
    g[:3] = 0.0
    v[:2] = 0.0
    coef = None if clip is None else torch.tensor(clip, dtype=torch.float32)
    (rp, bp), (rm, bm), (rv, bv) = kr.adamw_ref(p, g, m, v, lr, wd, b1, b2, eps, step, coef)

    def run(dt):
        q = torch.nn.Parameter(p.to(dt).clone())
        opt = torch.optim.AdamW([q], lr=kr._f32c(lr) if dt == torch.float64 else lr,
                                betas=(b1, b2), eps=eps, weight_decay=kr._f32c(wd) if dt == torch.float64 else wd,
                                foreach=False)
        opt.state[q] = dict(step=torch.tensor(float(step - 1)), exp_avg=m.to(dt).clone(), exp_avg_sq=v.to(dt).clone())
        q.grad = g.to(dt) * (1.0 if coef is None else coef.to(dt))
        opt.step()
        return q.detach(), opt.state[q]["exp_avg"], opt.state[q]["exp_avg_sq"]
    p64, m64, v64 = run(torch.float64)
    assert ((p64 - rp).abs() <= 1e-12 * rp.abs() + 1e-15).all() and (m64 - rm).abs().max() < 1e-15 and \
        (v64 - rv).abs().max() < 1e-15
    p32, m32, v32 = run(torch.float32)
    worst = max(kr.assert_within(p32, rp, bp, "p"), kr.assert_within(m32, rm, bm, "exp_avg"),
                kr.assert_within(v32, rv, bv, "exp_avg_sq"))
    assert worst <= HALF, worst


RESIZE_CASES = [(42, 42, 42), (42, 97, 42), (97, 131, 42), (30, 30, 42), (224, 224, 14), (64, 64, 512)]


@pytest.mark.parametrize("Hs,Ws,S", RESIZE_CASES, ids=str)
@pytest.mark.parametrize("u8", [False, True], ids=["f32src", "u8src"])
def test_resize_reference_is_torch_antialias_and_bound_holds(Hs, Ws, S, u8):
    """The restated triangle filter against F.interpolate(bilinear, antialias=True) in float64, MixUp / normalise / both
    layouts against their plain forms, and torch's fp32 interpolate as the emulation: worst ratio measured 0.35 for the copied
    (un-resized) sources and 0.03 for the resampled ones (the bound carries the fp32 tap positions' worst case, which a
    typical pixel stays far below)."""
    src = kr.image_source(3, Hs, Ws, u8, seed=Hs + Ws + S)
    ref, bound = kr.resize_ref(src, u8, S)
    x = src.permute(0, 3, 1, 2).double() / 255.0 if u8 else src.double()
    want = x if (Hs, Ws) == (S, S) else F.interpolate(x, size=(S, S), mode="bilinear", antialias=True, align_corners=False)
    assert (ref - want).abs().max() < 1e-6               # aten forms its scale and tap positions in fp32 even for double
    x32 = x.float()
    emu = x32 if (Hs, Ws) == (S, S) else F.interpolate(x32, size=(S, S), mode="bilinear", antialias=True, align_corners=False)
    mix = torch.tensor([1, 1, 0])
    out, ob = kr.preprocess_ref(src, u8, S, 14, 640, False, 0.5, 0.5, mix, 0.3, torch.float32)
    lam = torch.tensor(0.3)
    emu_out = ((lam * emu + (1 - lam) * emu[mix]) - 0.5) * torch.tensor(2.0)
    assert kr.assert_within(emu_out, out, ob, "fp32 interpolate + mixup + normalise") <= HALF
    if S % 14 == 0 and S <= 42:
        pm, pb = kr.preprocess_ref(src, u8, S, 14, 640, True, 0.5, 0.5, mix, 0.3, torch.float32)
        g = S // 14
        assert pm.shape == (3 * g * g, 640) and bool((pm[:, 588:] == 0).all()) and bool((pb[:, 588:] == 0).all())
        assert torch.equal(pm[:, :588].reshape(3, g, g, 3, 14, 14).permute(0, 3, 1, 4, 2, 5).reshape(3, 3, S, S), out)


def test_resize_bound_catches_unnormalised_weights():
    """Dropping the division by the weights' total (the `* inv_total` mutant) scales a 3x down-sampled image by 3."""
    src = kr.image_source(2, 97, 131, False, seed=5)
    ref, bound = kr.resize_ref(src, False, 42)
    assert kr.worst_ratio(ref * (131 / 42), ref, bound) > 1e3


@pytest.mark.parametrize("case", kr.AUG_CASES, ids=lambda c: c[0])
def test_aug_reference_matches_fp32_oracle_and_hue_cap_holds(case):
    """The float64 restatement of the header's augmentation against oracle/preprocess_oracle.py (fp32 torch, torch's own
    antialiased resize) as the emulation, on the very inputs the GPU test uses: worst ratio measured 0.25 (the same with and
    without the hue-excused pixels: on these inputs the rule excuses nothing that is out of bound), and the excused share of
    every IMAGE is under the 1 % cap (measured: at most 0.35 % of an image; the one record that rotates and jitters has no
    hue step, because the zero corners of a rotation alone are 2 % of excusable pixels)."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location(
        "preprocess_oracle", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle",
                                          "preprocess_oracle.py"))
    po = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(po)
    name, u8, code, _, S, P, Kp, patch = case
    src, tab = kr.aug_case_inputs(name)
    out, bound, gm, gb, mask = kr.aug_ref(src, u8, S, tab, 0.5, 0.5, torch.float32)
    share = mask.float().mean((1, 2))                    # per image: records without a hue step would dilute a case mean
    assert share.max().item() <= kr.HUE_EXCUSED_CAP, share.tolist()
    params = [dict(flip=t["flip"] != 0, cos=t["cos"], sin=t["sin"], brightness=t["brightness"], contrast=t["contrast"],
                   saturation=t["saturation"], hue=t["hue"], order=t["order"] if t["order"][0] >= 0 else None)
              for t in tab]
    emu = po.augment_transform(src, S, params)
    keep = ~mask[:, None].expand_as(out)
    r = kr.worst_ratio(emu[keep], out[keep], bound[keep])
    assert r <= HALF, r
    assert bool((gm[[0, 1, 2, 3, 7]] == 0).all()) and bool((gb[[0, 1, 2, 3, 7]] == 0).all())
    # flip mutant S - 1 - x -> S - x: the flipped records move by one pixel
    shifted = torch.roll(out, 1, dims=-1)
    assert kr.worst_ratio(shifted[1][keep[1]], out[1][keep[1]], bound[1][keep[1]]) > 10


# ---------------------------------------------------------------------------------------------------------------
# the kernels only the encoder calls (tests/test_kernel_edges_internal_gpu.py)
# ---------------------------------------------------------------------------------------------------------------
def _pos_case(g0, gh, gw, D, seed, prior_scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(gh * gw, D, generator=g), torch.randn(g0 * g0, D, generator=g) * prior_scale


def test_pos_resize_bwd_reference_is_the_autograd_of_bicubic_interpolate():
    """The dense float64 resize matrix, transposed, against float64 autograd of F.interpolate(bicubic) on every grid."""
    for g0, gh, gw in kr.POS_BWD_GRIDS:
        dout, prior = _pos_case(g0, gh, gw, 5, 0)
        t = torch.randn(g0 * g0, 5, dtype=torch.float64, requires_grad=True)
        kr.pos_resize_ref(t, g0, gh, gw).backward(dout.double())
        ref, _ = kr.pos_resize_bwd_ref(dout, g0, gh, gw, prior)
        assert (t.grad + prior.double() - ref).abs().max().item() < 1e-13, (g0, gh, gw)
        fwd = kr.resize_matrix(g0, gh)                     # and the matrix itself against the forward reference
        assert fwd.sum(1).sub(1).abs().max().item() < 1e-14


def test_pos_resize_bwd_constant_is_measured_from_the_emulation():
    """POS_BWD_C: the per-weight excess of the fp32 polynomials over the derived coordinate slack, measured on the axes the
    GPU test uses (11.6), times 2 to 4.  The emulation then sits at 0.16 of the bound at the worst (asserted <= 0.5) for
    zero and normal priors, D = 5 and 144; without the constant it leaves the bound (1.85)."""
    excess = max(kr.pos_resize_weight_excess(g0, n) for g0, gh, gw in kr.POS_BWD_GRIDS for n in (gh, gw))
    assert 2.0 * excess <= kr.POS_BWD_C <= 4.0 * excess, excess
    worst, worst0 = 0.0, 0.0
    for g0, gh, gw in kr.POS_BWD_GRIDS:
        for seed in range(3):
            for D in (5, 144):
                for ps in (0.0, 1.0):
                    dout, prior = _pos_case(g0, gh, gw, D, seed, ps)
                    emu = kr.pos_resize_bwd_emulate(dout, g0, gh, gw, prior)
                    ref, bound = kr.pos_resize_bwd_ref(dout, g0, gh, gw, prior)
                    worst = max(worst, kr.assert_within(emu, ref, bound, f"emulation {g0}->{gh}x{gw}"))
                    worst0 = max(worst0, kr.worst_ratio(emu, ref, kr.pos_resize_bwd_ref(dout, g0, gh, gw, prior, c=0.0)[1]))
    assert 0.05 < worst <= 0.5, worst
    assert worst0 > 1.0, worst0


def test_pos_resize_bwd_relative_form_cannot_hold_small_weights():
    """Why the bound is not (terms + c) 2^-24 sum|w||dout|: at 27 -> 1 x 5 the fp32 weights of 0.02 to 0.2 are off by 5 to
    22 2^-24 each, so that form needs c above 100 for the emulation (and more the larger g0)."""
    g0, gh, gw = 27, 1, 5
    need = 0.0
    for seed in range(3):
        dout, prior = _pos_case(g0, gh, gw, 5, seed, 0.0)
        emu = kr.pos_resize_bwd_emulate(dout, g0, gh, gw, prior).double()
        Ry, Rx = kr.resize_matrix(g0, gh), kr.resize_matrix(g0, gw)
        G = dout.double().view(gh, gw, 5)
        ref = torch.einsum("ya,yxd,xb->abd", Ry, G, Rx).reshape(g0 * g0, 5)
        mag = torch.einsum("ya,yxd,xb->abd", Ry.abs(), G.abs(), Rx.abs()).reshape(g0 * g0, 5)
        live = mag > 0
        need = max(need, ((emu - ref).abs()[live] / (kr.EPS32 * mag[live])).max().item())
    assert need > 100.0, need


def test_pos_resize_bwd_bound_catches_a_narrow_scan():
    """tap_range scanning +-1 source rows instead of +-3 (borders widened as the kernel does) drops whole contributions
    on the steep upscale: outputs 30..36 of 37 reach table row 0 through their first tap.  Far outside the bound."""
    g0, gh, gw = 2, 37, 5
    dout, prior = _pos_case(g0, gh, gw, 5, 0)
    ref, bound = kr.pos_resize_bwd_ref(dout, g0, gh, gw, prior)
    narrow, Rx = kr.resize_matrix(g0, gh), kr.resize_matrix(g0, gw)
    oy = torch.arange(gh)
    for ty in range(g0):
        lo = 0 if ty == 0 else math.floor((ty - 1 + 0.5) * gh / g0 - 0.5) - 1
        hi = gh - 1 if ty == g0 - 1 else math.ceil((ty + 1 + 0.5) * gh / g0 - 0.5) + 1
        narrow[(oy < lo) | (oy > hi), ty] = 0.0
    assert not torch.equal(narrow, kr.resize_matrix(g0, gh))
    got = torch.einsum("ya,yxd,xb->abd", narrow, dout.double().view(gh, gw, 5), Rx).reshape(g0 * g0, 5) + prior.double()
    assert kr.worst_ratio(got, ref, bound) > 20


@pytest.mark.parametrize("tdt", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("kind", ["gauss", "big", "equal"])
def test_pool_attn_bounds_hold_for_the_emulation_and_catch_mutants(kind, tdt):
    """pool_attn_emulate (the kernels' recipe in torch fp32) inside every bound: at most 0.5 for the fp32 quantities
    (probs <= 0.12, dq <= 0.03, fp32 out <= 0.02; fp32 dkv 0.5 = the one rounding of dV), at most 1 for 16-bit stores
    (their own half ulp).  Outside: the backward without `- dot`, the scale rsqrt(DP) for rsqrt(dh), a truncating store."""
    worst = [0.0] * 4
    for dh, DP in ((8, 16), (72, 80)):
        for N in (1, 25, 257, 1364):
            B, H = 2, 3
            q, K, V, do = kr.pool_inputs(kind, B, H, N, dh, DP, tdt, 1)
            (Pr, bP), (o, bo) = kr.pool_attn_fwd_ref(q, K, V, H, dh, tdt)
            P32 = Pr.float()
            (dkv, bkv), (dq, bq) = kr.pool_attn_bwd_ref(q, K, V, P32, do, H, dh, tdt)
            eP, eo, ekv, edq = kr.pool_attn_emulate(q, K, V, do, H, dh, tdt, P32)
            what = f"{kind} dh={dh} N={N}"
            rs = [kr.assert_within(eP, Pr, bP, what + " probs"), kr.assert_within(eo, o, bo, what + " out"),
                  kr.assert_within(ekv, dkv, bkv, what + " dkv"), kr.assert_within(edq, dq, bq, what + " dq")]
            worst = [max(a, b) for a, b in zip(worst, rs)]
            assert (Pr.sum(-1) - 1).abs().max().item() < 1e-12
            if N < 25 or kind != "gauss":
                continue
            # mutants, in float64 so that only the mutation differs
            scale, bad = dh ** -0.5, DP ** -0.5
            S = torch.einsum("hd,bhnd->bhn", q.double().view(H, dh), K.double()[..., :dh])
            assert kr.worst_ratio(torch.softmax(S * bad, -1), Pr, bP) > 100, what
            dp = torch.einsum("bhd,bhnd->bhn", do.double().view(B, H, dh), V.double()[..., :dh])
            ds_mut = P32.double() * dp * scale                                    # `- dot` dropped
            dq_mut = torch.einsum("bhn,bhnd->bhd", ds_mut, K.double()[..., :dh]).reshape(B, H * dh)
            assert kr.worst_ratio(dq_mut, dq, bq) > 100, what
            if tdt != torch.float32:
                assert kr.worst_ratio(kr.truncate_to(dkv, tdt), dkv, bkv) > 1.5, what
    lim = 0.5 if tdt == torch.float32 else 1.0
    assert worst[0] <= 0.5 and worst[3] <= 0.5 and worst[1] <= lim and worst[2] <= lim, worst


def test_pool_attn_reference_is_the_autograd_of_softmax_attention():
    B, H, N, dh, DP = 2, 3, 33, 24, 32
    q, K, V, do = kr.pool_inputs("gauss", B, H, N, dh, DP, torch.float32, 4)
    q64 = q.double().view(H, dh).requires_grad_(True)
    K64, V64 = K.double()[..., :dh].requires_grad_(True), V.double()[..., :dh].requires_grad_(True)
    Pr = torch.softmax(torch.einsum("hd,bhnd->bhn", q64, K64) * dh ** -0.5, -1)
    out = torch.einsum("bhn,bhnd->bhd", Pr, V64).reshape(B, H * dh)
    out.backward(do.double())
    (rP, _), (ro, _) = kr.pool_attn_fwd_ref(q, K, V, H, dh, torch.float32)
    assert (rP - Pr).abs().max().item() < 1e-14 and (ro - out).abs().max().item() < 1e-13
    # the backward reference takes the probabilities in fp32: compare at that precision
    (dkv, _), (dq, _) = kr.pool_attn_bwd_ref(q, K, V, Pr.detach().float(), do, H, dh, torch.float32)
    tok = lambda t: t.permute(0, 2, 1, 3).reshape(B * N, H * dh)
    assert (dkv - torch.cat([tok(K64.grad), tok(V64.grad)], 1)).abs().max().item() < 1e-6
    assert (dq.view(B, H, dh).sum(0) - q64.grad).abs().max().item() < 1e-5


def test_sum_bound_holds_for_any_fp32_order_and_split3_reconstructs():
    """sum_ref: a sequential fp32 chain and a pairwise tree of 1152 terms inside n 2^-24 sum|terms| (measured 0.01 to
    0.03), a sum that loses one term outside.  split3: hi + lo within 2^-17 |x| for normal x, exact layout segments."""
    g = torch.Generator().manual_seed(0)
    t = torch.randn(1152, 65, generator=g)
    prior = torch.randn(65, generator=g)
    ref, bound = kr.sum_ref(t, prior)
    seq = prior.clone()
    for i in range(t.shape[0]):
        seq = seq + t[i]
    tree = t.clone()
    while tree.shape[0] > 1:
        if tree.shape[0] % 2:
            tree = torch.cat([tree, torch.zeros(1, tree.shape[1])])
        tree = tree[0::2] + tree[1::2]
    assert kr.assert_within(seq, ref, bound, "sequential") <= 0.5
    assert kr.assert_within(tree[0] + prior, ref, bound, "tree") <= 0.5
    assert kr.worst_ratio(seq - t[-1], ref, bound) > 10
    rv, bv = kr.vecmat_ref(t[:, 0], t, None)
    assert kr.assert_within((t[:, :1] * t).sum(0), rv, bv, "vecmat") <= 0.5
    x = torch.cat([torch.randn(4096, generator=g) * torch.logspace(-20, 20, 4096), kr.split3_special_values()])
    hi, lo = kr.split3_ref(x)
    normal = (x.abs() >= 2.0 ** -100) & torch.isfinite(hi.float())
    rec = hi.double() + lo.double()
    assert bool(((rec - x.double()).abs()[normal] <= 2.0 ** -17 * x.double().abs()[normal]).all())
    lay = kr.split3_layout(x[:18].view(2, 9), 16, 1, False)
    assert lay.shape == (2, 48) and torch.equal(lay[:, 16:25], lo[:18].view(2, 9)) and bool((lay[:, 9:16] == 0).all())
    assert torch.equal(kr.split3_layout(x[:18].view(2, 9), 16, 0, True)[4:6, :9], lo[:18].view(2, 9))
