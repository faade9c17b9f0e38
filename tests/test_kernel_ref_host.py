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
