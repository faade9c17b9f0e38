"""GPU: the non-finite propagation contract of DESIGN.md ("Non-finite values") on the kernels of the training path.

`siglip_amd.GradScaler` decides whether a step is skipped from one thing, whether the sum of squares of the gradients that
reach FusedAdamW is finite, so an inf or NaN anywhere in a forward or backward pass has to reach every gradient that
depends on it (rule 1, no swallowing), and a corrupt image or row must not change one bit of another's outputs (rule 2,
no spreading).  Each test plants one NaN, +inf or -inf in the middle of one operand and compares, element by element,
with the float64 reference of the same operation on the same poisoned input: tests/nonfinite_util.py holds the driver,
the rules and the case tables, tests/test_nonfinite_host.py the conditions on the references alone.  Sites and values
are looped inside a test so that the clean launch is shared; every test prints its number of (site, value) cases and
its largest excused share (pytest -s).

The shapes are the smallest at which each code path still has a partial tile:
  attention  B = 2, H = 2; N = 33: one query tile, one key in the second 32-key half; N = 130: a third 64-key tile
             holding two keys, across the 128-row head block; dh = 8 -> DP16, dh = 72 -> DP80.  The poisoned head is
             (b = 1, h = 0); everything of the other three heads has to keep the clean launch's bits.
  LayerNorm  M = 5 (a second, partial workgroup of 4 rows); D = 4, 516, 1152: one float4, and both wider instantiations.
  NT GEMM    M = 333 (128-row tiles) and 2333 (256-row tiles), both with a partial last tile; N = 264 (a partial column
             tile), K = 72 (k = 71 lies in the partial K step); one launch at the encoder's width N = 1152, which the
             dispatch sends to the 384 x 192 tile.
"""
import pytest
import torch

import kernel_ref as kr
import nonfinite_util as nf
from attn_util import DEV, Guarded, P, ok, rup, run_attention, stream, tdt_of
from kernel_ref import BF16
from op_runners import (padded, run_gemm_nt, run_gemm_nt_qkv, run_gemm_tn, run_layernorm, run_pool_attn_bwd,
                        run_pool_attn_fwd)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib(hiplib):
    assert torch.cuda.is_available()
    return hiplib


def on_device(inputs):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in inputs.items()}


def on_host(inputs):
    return {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in inputs.items()}


def checked(outs, what, poisoned):
    """The guard bands of every output (always) and, for a clean launch, that every element was written; the bodies."""
    got = {}
    for name, g in outs.items():
        g.check(f"{what} {name}", written=not poisoned)
        got[name] = g.got()
    return got


# =========================================================================================================
# attention forward + backward (the backward consumes the forward's own output)
# =========================================================================================================
@pytest.mark.parametrize("N,dh", nf.ATTN_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("layout", ["token", "head"])
@pytest.mark.parametrize("dtype", nf.ATTN_DTYPES, ids=lambda d: kr.DT_NAME[d])
def test_attention_fwd_bwd(lib, dtype, layout, N, dh):
    """q, k, v, dout of head (1, 0) poisoned at (0, 0), (N - 1, dh - 1) and, for N = 130, (64, dh - 1): O, lse, dQ, dK,
    dV.  The reference's granularity has to come back: a poisoned q row gives that row of O, lse and dQ and all of dK
    and dV; a poisoned v column that column of O, nothing of dV, all of dQ and dK; a poisoned dout column that column
    of dV; nothing in the other three heads (tests/test_nonfinite_host.py asserts that of the reference)."""
    inp = on_device(nf.attn_inputs(dtype, N, dh))

    def run(d, poisoned):
        O, lse, dQ, dK, dV = run_attention(lib, dtype, layout, d["q"], d["k"], d["v"], d["dout"], written=not poisoned)
        return dict(O=O, lse=lse, dQ=dQ, dK=dK, dV=dV)
    nf.drive(f"attention {kr.DT_NAME[dtype]} {layout} N={N} dh={dh}", run, nf.attn_ref, inp, nf.attn_sites(inp))


# =========================================================================================================
# LayerNorm forward + backward
# =========================================================================================================
@pytest.mark.parametrize("dres", [True, False], ids=["dres", "no_dres"])
@pytest.mark.parametrize("dtype", nf.LN_DTYPES, ids=lambda d: kr.DT_NAME[d])
@pytest.mark.parametrize("D", nf.LN_D, ids=lambda d: f"D{d}")
def test_layernorm_fwd_bwd(lib, D, dtype, dres):
    """x, dy at rows {0, 4} x columns {0, D - 1} and gamma at {0, D - 1}: y, mean, rstd, dx (fp32 and the low-precision
    copy, with and without the residual gradient), dgamma, dbeta.  x poisons its row of y, mean, rstd and dx and all of
    dgamma; dy its row of dx and one column each of dgamma and dbeta; gamma its column of y and all of dx."""
    inp = on_device(nf.ln_inputs(D, dtype, dres))
    what = f"layernorm {kr.DT_NAME[dtype]} D={D}" + (" dres" if dres else "")

    def run(d, poisoned):
        o = run_layernorm(lib, d["x"], d["gamma"], d["beta"], d["dy"], d["dres"], dtype, dtype, dtype)
        got = checked(o, what, poisoned)
        return {k: (v[0] if k in ("mean", "rstd", "dgamma", "dbeta") else v) for k, v in got.items()}
    nf.drive(what, run, nf.ln_ref, inp, nf.ln_sites(D))


# =========================================================================================================
# NT GEMM, every epilogue of the edge tests
# =========================================================================================================
def nt_case(lib, dtype, M, epi, N=nf.NT_N, K=nf.NT_K):
    inp = on_device(nf.nt_inputs(dtype, M, epi, N, K))
    what = f"gemm_nt {kr.DT_NAME[dtype]} M={M} N={N} K={K} epi={epi}"

    def run(d, poisoned):
        # the leading dimensions of the edge tests, NaN in the slack: a read past the logical width poisons everything
        A, B = padded(d["A"], K + 8), padded(d["B"], K + 8)
        res = padded(d["res"], N + 8) if "res" in d else None
        aux = padded(d["aux"], N + 24) if "aux" in d else None
        out, out2 = run_gemm_nt(lib, dtype, M, N, K, epi, A, B, d.get("bias"), res, aux, d.get("pos"))
        return checked(dict(out=out, out2=out2) if out2 is not None else dict(out=out), what, poisoned)
    nf.drive(what, run, nf.nt_ref(epi), inp, nf.nt_sites(M, epi, N, K))


@pytest.mark.parametrize("epi", nf.NT_EPIS, ids=lambda e: f"epi{e}")
@pytest.mark.parametrize("M", nf.NT_M, ids=lambda m: f"M{m}")
@pytest.mark.parametrize("dtype", nf.NT_DTYPES, ids=lambda d: kr.DT_NAME[d])
def test_gemm_nt_epilogues(lib, dtype, M, epi):
    """A[i, k] poisons row i of the output, B[j, k] column j (k = 0 and k = 71, i and j in the first and in the last,
    partial tile), bias[j] column j, and one element each the residual (epilogue 2), the saved GELU operand (4: the
    output is dY . gelu'(u), and gelu'(+-inf) is s (1 - s) . inf = NaN) and the position row (5: every row that reads
    it).  Epilogue 1 has two outputs, the pre-activation and its GELU; gelu(-inf) = -inf . 0 is NaN in the kernel and in
    the reference alike."""
    nt_case(lib, dtype, M, epi)


def test_gemm_nt_production_width(lib):
    """N = 1152 with a plain store and M >= 2048: the 384 x 192 tile."""
    nt_case(lib, BF16, *[nf.NT_WIDE[i] for i in (0, 3, 1, 2)])


@pytest.mark.parametrize("shape", nf.QKV_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("dtype", nf.NT_DTYPES, ids=lambda d: kr.DT_NAME[d])
def test_gemm_nt_qkv_scatter(lib, dtype, shape):
    """The QKV scatter epilogue on both kernel generations (M = 100 and 2100), hd = 40 padded to 48: A's row poisons
    that token in q, k and v of every head, B's row and the bias element one column of one head; the pad columns are
    written as zero whatever the input holds."""
    batch, tokens, heads, hd = shape
    hdp = (hd + 15) // 16 * 16
    D = heads * hd
    inp = on_device(nf.qkv_inputs(dtype, *shape))
    what = f"gemm_nt qkv {kr.DT_NAME[dtype]} {shape}"

    def run(d, poisoned):
        out = run_gemm_nt_qkv(lib, dtype, padded(d["A"], D + 8), padded(d["B"], D + 8), d["bias"], batch, tokens, heads, hd, hdp)
        got = checked(dict(qkv=out), what, poisoned)["qkv"].view(3, batch, heads, tokens, hdp)
        assert bool((got[..., hd:] == 0).all()), f"{what}: pad columns must be written as zero"
        return dict(qkv=got[..., :hd])
    nf.drive(what, run, nf.qkv_ref(*shape), inp, nf.qkv_sites(*shape))


# =========================================================================================================
# TN GEMM (dW): every split route
# =========================================================================================================
def tn_case(lib, dtype, route, accumulate):
    name, Mred, N2, splits, ws_bytes, fixed_order = route
    N1 = nf.TN_N
    inp = on_device(nf.tn_inputs(dtype, Mred, N2, accumulate))
    what = f"gemm_tn {kr.DT_NAME[dtype]} {name} acc={accumulate}"
    lda, ldb, ldo = N1 + 8, (N2 + 7) // 8 * 8 + 8, (N2 + 3) // 4 * 4 + 4

    def run(d, poisoned):
        out = run_gemm_tn(lib, dtype, padded(d["A"], lda), padded(d["B"], ldb), Mred, N1, N2, ldo, splits, accumulate,
                          d["prior"], ws_bytes)
        return checked(dict(out=out), what, poisoned)
    nf.drive(what, run, nf.tn_ref, inp, nf.tn_sites(Mred, N2), bounds=None if fixed_order else nf.tn_bounds)


@pytest.mark.parametrize("accumulate", [0, 1], ids=["store", "accumulate"])
@pytest.mark.parametrize("route", nf.TN_ROUTES, ids=lambda r: r[0])
@pytest.mark.parametrize("dtype", nf.TN_DTYPES, ids=lambda d: kr.DT_NAME[d])
def test_gemm_tn_routes(lib, dtype, route, accumulate):
    """A[m, i] poisons row i of dW and B[m, j] column j, with m in the first and in the last split, on the small-tile
    kernel (Mred = 2047; one split, and three that add with fp32 atomics) and on the 256-row kernel (Mred = 2048, which
    splits on its own: atomics without scratch, slabs summed in a fixed order with it).  Where the splits add with atomics
    the order of the additions is not fixed, so rule 2 holds the independent elements to the float64 bound of
    test_gemm_tn_ws_fallbacks_guard (kernel_ref.gemm_tn_ref) and not to the clean launch's bits; the fixed-order routes
    are held to bits."""
    tn_case(lib, dtype, route, accumulate)


@pytest.mark.parametrize("accumulate", [0, 1], ids=["store", "accumulate"])
@pytest.mark.parametrize("route", nf.TN_FALLBACKS, ids=lambda r: r[0])
def test_gemm_tn_ws_atomic_fallbacks(lib, route, accumulate):
    """sgl_op_gemm_tn_ws with scratch too small for the slabs and with N2 % 4 != 0: the atomic fallbacks, independent
    elements held to the float64 bound (see test_gemm_tn_routes)."""
    tn_case(lib, BF16, route, accumulate)


# =========================================================================================================
# MX-fp8: LayerNorm -> MX operand, quantize -> block-scaled GEMM
# =========================================================================================================
@pytest.mark.parametrize("D", nf.LN_MX_D, ids=lambda d: f"D{d}")
def test_layernorm_fwd_mx(lib, D):
    """x poisons its row, gamma the 32-block of its column in every row: a block that holds a non-finite value is scale
    byte 0xFF and 0x7F elements as a whole, which the reference quantiser reproduces, so the comparison is on
    the dequantised operand; the bytes of every non-finite block are asserted as well."""
    import mx_ref
    Kp = nf.mx_kpad(D)
    inp = on_device(nf.ln_mx_inputs(D))

    def run(d, poisoned):
        q = torch.full((nf.LN_M, Kp), 0xAB, dtype=torch.uint8, device=DEV)
        s = torch.full((nf.LN_M, Kp // 32), 0xAB, dtype=torch.uint8, device=DEV)
        ok(lib.sgl_op_layernorm_fwd_mx(P(d["x"]), P(d["gamma"]), P(d["beta"]), P(q), P(s), nf.LN_M, D, Kp, nf.LN_EPS, stream()))
        torch.cuda.synchronize()
        deq = mx_ref.dequantize(q, s)
        bad = nf.nonfinite(deq).view(nf.LN_M, Kp // 32, 32).any(-1)
        assert bool((s[bad] == 0xFF).all()) and bool((q.view(nf.LN_M, Kp // 32, 32)[bad] == 0x7F).all()), \
            "a non-finite block must be scale byte 0xFF and 0x7F elements"
        assert bool((s[~bad] != 0xFF).all())
        return dict(deq=deq)
    nf.drive(f"layernorm_fwd_mx D={D}", run, nf.ln_mx_ref, inp, nf.ln_mx_sites(D), to_ref=on_host)


def test_quantize_mxfp8_gemm_nt_mx(lib):
    """x [333, 72] quantised (Kp = 128) and multiplied with a quantised weight [264, 72], fp32 residual epilogue: x[i, k]
    poisons row i of the output, every other row keeps its bits."""
    M, N, K, Kp = nf.MX_M, nf.MX_N, nf.MX_K, nf.mx_kpad(nf.MX_K)
    inp = on_device(nf.mx_gemm_inputs())

    def quant(x):
        q = torch.full((x.shape[0], Kp), 0xAB, dtype=torch.uint8, device=DEV)
        s = torch.full((x.shape[0], Kp // 32), 0xAB, dtype=torch.uint8, device=DEV)
        ok(lib.sgl_op_quantize_mxfp8(P(x), kr.F32, x.stride(0), x.shape[0], K, Kp, P(q), P(s), stream()))
        return q, s

    def run(d, poisoned):
        (aq, as_), (bq, bs) = quant(d["x"]), quant(d["w"])
        out = Guarded(M, N, N, torch.float32)
        ok(lib.sgl_op_gemm_nt_mx(P(aq), P(as_), P(bq), P(bs), M, N, Kp, 2, out.ptr, N, None, P(d["bias"]), P(d["res"]),
                                 N, 1, 1, 8, 8, 1, stream()))
        torch.cuda.synchronize()
        return checked(dict(out=out), "gemm_nt_mx", poisoned)
    nf.drive("quantize_mxfp8 + gemm_nt_mx", run, nf.mx_gemm_ref, inp, nf.mx_gemm_sites(), to_ref=on_host)


# =========================================================================================================
# pooling-head attention (one query per head), forward + backward from the forward's own probabilities
# =========================================================================================================
@pytest.mark.parametrize("dims", nf.POOL_DIMS, ids=lambda d: f"dh{d[0]}_dp{d[1]}")
@pytest.mark.parametrize("dtype", nf.POOL_DTYPES, ids=lambda d: kr.DT_NAME[d])
def test_pool_attention_fwd_bwd(lib, dtype, dims):
    """B = 2, H = 2, N = 100, DP 16 and 96.  The query is shared by the images, so a poisoned q element reaches both; K, V
    and dout of image 1, head 0 (first and last token) must leave image 0 and head 1 with the clean launch's bits.  The
    softmax maximum is formed with fmaxf / wave_max, which drop a NaN: the NaN has to arrive through exp and the row sum."""
    dh, DP = dims
    B, H, N = nf.POOL_B, nf.POOL_H, nf.POOL_N
    inp = on_device(nf.pool_inputs(dtype, dh, DP))
    what = f"pool_attn {kr.DT_NAME[dtype]} dh={dh}"

    def run(d, poisoned):
        out, probs = run_pool_attn_fwd(lib, dtype, d["q"], d["K"], d["V"], B, H, N, dh, DP)
        dkv, dq = run_pool_attn_bwd(lib, dtype, d["q"], d["K"], d["V"], probs.ptr, d["dout"], B, H, N, dh, DP)
        return checked(dict(out=out, probs=probs, dkv=dkv, dq=dq), what, poisoned)
    nf.drive(what, run, nf.pool_ref(dh), inp, nf.pool_sites(inp, dh))


# =========================================================================================================
# head kernels: gate_mul, l2norm_tmean
# =========================================================================================================
@pytest.mark.parametrize("dtype", nf.GATE_DTYPES, ids=lambda d: kr.DT_NAME[d])
def test_gate_mul_fwd_bwd(lib, dtype):
    """y = sigmoid(g) x, dg, dx at one vector and at three blocks plus a vector: first, last and a tail element of x and
    dy with all three values, of the gate with NaN (a gate at +-inf is sigmoid 1 or 0: everything stays finite)."""
    tdt = tdt_of(dtype)
    for n in nf.gate_sizes(dtype):
        inp = on_device(nf.gate_inputs(dtype, n))
        what = f"gate_mul {kr.DT_NAME[dtype]} n={n}"

        def run(d, poisoned):
            y, dg, dx = (Guarded(1, n, rup(n, 8), tdt) for _ in range(3))
            ok(lib.sgl_op_gate_mul(P(d["gate"]), P(d["x"]), y.ptr, n, dtype, stream()))
            ok(lib.sgl_op_gate_mul_bwd(P(d["dy"]), P(d["gate"]), P(d["x"]), dg.ptr, dx.ptr, n, dtype, stream()))
            torch.cuda.synchronize()
            return {k: v[0] for k, v in checked(dict(y=y, dg=dg, dx=dx), what, poisoned).items()}
        nf.drive(what, run, nf.gate_ref, inp, nf.gate_sites(n))


@pytest.mark.parametrize("shape", nf.L2_SHAPES, ids=str)
def test_l2norm_tmean_fwd_bwd(lib, shape):
    """A poisoned frame element reaches its image's mean, its own inv_norm and its frame of df (the backward reads the
    forward's own inv_norm); the other images and frames keep their bits.  f = +-inf gives inv_norm = 0 and 0 * finite
    zeros in the other columns of the mean: those are the excused half."""
    B, T, D = shape
    inp = on_device(nf.l2_inputs(B, T, D))
    what = f"l2norm_tmean {shape}"

    def run(d, poisoned):
        out, inv, df = Guarded(B, D, D, torch.float32), Guarded(1, B * T, rup(B * T, 8), torch.float32), \
            Guarded(B * T, D, D, torch.float32)
        ok(lib.sgl_op_l2norm_tmean_fwd(P(d["f"]), out.ptr, inv.ptr, B, T, D, stream()))
        inv_dev = inv.got().reshape(-1).contiguous()
        ok(lib.sgl_op_l2norm_tmean_bwd(P(d["f"]), P(inv_dev), P(d["dout"]), df.ptr, B, T, D, stream()))
        torch.cuda.synchronize()
        got = checked(dict(out=out, inv_norm=inv, df=df), what, poisoned)
        got["inv_norm"] = got["inv_norm"][0]
        return got
    nf.drive(what, run, nf.l2_ref(B, T), inp, nf.l2_sites(B, T, D))


@pytest.mark.parametrize("accumulate", [0, 1], ids=["store", "accumulate"])
@pytest.mark.parametrize("dtype", nf.DW_DTYPES, ids=lambda d: kr.DT_NAME[d])
def test_dwconv3x3_and_wgrad(lib, dtype, accumulate):
    """x reaches the 3 x 3 neighbourhood of its pixel in its channel of y, and that channel's column of dw10; dy its
    channel's column of dw10 (all ten rows); the bias its channel of y.  Other channels and the other image keep their
    bits."""
    tdt = tdt_of(dtype)
    for B, gh, gw, E in nf.dw_shapes(dtype):
        inp = on_device(nf.dw_inputs(dtype, B, gh, gw, E, accumulate))
        what = f"dwconv3x3 {kr.DT_NAME[dtype]} {(B, gh, gw, E)} acc={accumulate}"
        npix = B * gh * gw
        ppb = -(-npix // min(npix, 512))
        need = -(-npix // ppb) * 10 * E * 4
        assert need <= lib.sgl_op_dwconv3x3_wgrad_scratch_bytes(B, gh, gw, E)

        def run(d, poisoned):
            y = Guarded(npix, E, E, tdt)
            dw = Guarded(10, E, E, torch.float32, prior=d["prior"])
            scratch = torch.empty(need // 4, device=DEV)
            ok(lib.sgl_op_dwconv3x3(P(d["x"]), dtype, P(d["w9"]), P(d["bias"]), y.ptr, B, gh, gw, E, 0, stream()))
            ok(lib.sgl_op_dwconv3x3_wgrad(P(d["x"]), P(d["dy"]), dtype, dw.ptr, accumulate, P(scratch), need, B, gh, gw, E,
                                          stream()))
            torch.cuda.synchronize()
            got = checked(dict(y=y, dw10=dw), what, poisoned)
            return dict(y=got["y"].view(B, gh, gw, E), dw10=got["dw10"])
        nf.drive(what, run, nf.dw_ref, inp, nf.dw_sites(B, gh, gw, E))


@pytest.mark.parametrize("shape", nf.SEG_SHAPES, ids=str)
def test_seg_loss_fwd_bwd(lib, shape):
    """A NaN logit of image 1 makes the bce, p t and p partials of the 8-row chunks that read it bilinearly non-finite
    (the kernel's fmaxf(z, 0) drops the NaN; - z t and log1p carry it), never the sum of t, and through the dice sums all
    of image 1's gradient; a poisoned target pixel likewise.  Images 0 and 2 keep their bits.  The backward gets the
    caller's fold of the forward's own partials, as the head does."""
    g, S = shape
    B = nf.SEG_B
    inp = on_device(nf.seg_inputs(g, S))
    chunks = lib.sgl_op_seg_loss_chunks(S)
    what = f"seg_loss {shape}"

    def run(d, poisoned):
        part = Guarded(B * chunks, 4, 4, torch.float32)
        ok(lib.sgl_op_seg_loss_fwd(P(d["lr"]), P(d["tgt"]), part.ptr, B, g, S, stream()))
        torch.cuda.synchronize()
        sums = part.got().view(B, chunks, 4).double().sum(1).float().contiguous()
        dl = Guarded(B * g, g, g, torch.float32)
        ok(lib.sgl_op_seg_loss_bwd(P(d["lr"]), P(d["tgt"]), P(sums), P(d["coef"]), dl.ptr, B, g, S, nf.SEG_EPS, stream()))
        torch.cuda.synchronize()
        got = checked(dict(partial=part, dlogits=dl), what, poisoned)
        return dict(partial=got["partial"].view(B, chunks, 4), dlogits=got["dlogits"].view(B, g, g))
    nf.drive(what, run, nf.seg_ref, inp, nf.seg_sites(g, S), to_ref=on_host)      # index_add_ is ordered on the CPU only


@pytest.mark.parametrize("case", nf.SEG_EX_CASES, ids=str)
def test_seg_loss_ex_fwd_bwd(lib, case):
    """The enhanced loss with every term on (focal, boundary, smoothness): a NaN logit of image 1 reaches the eight-row
    chunks whose pixels, or whose pixels' smoothness pairs, read it (every sum but sum t), and through the folded sums
    all of image 1's gradient; image 0 keeps its bits.  The runner is tests/test_seg_loss_ex_gpu.py's (guarded arenas)."""
    import seg_loss_ex_ref as sr
    from test_seg_loss_ex_gpu import raw_bwd, raw_fwd
    B, g, S = case
    inp = on_device(nf.seg_ex_inputs(*case))

    def run(d, poisoned):
        part = raw_fwd(lib, d["lr"], d["tgt"], B, g, S, nf.SEG_EX_TERMS)
        dl = raw_bwd(lib, d["lr"], d["tgt"], sr.fold(part), d["coef"], B, g, S, nf.SEG_EX_TERMS, eps=nf.SEG_EX_EPS,
                     smooth=nf.SEG_EX_EPS)
        return dict(partial=part, dlogits=dl)
    nf.drive(f"seg_loss_ex {case}", run, nf.seg_ex_ref, inp, nf.seg_ex_sites(*case), to_ref=on_host)


# =========================================================================================================
# sums and copies: colsum, batch_sum, vecmat, add_f32, split3
# =========================================================================================================
@pytest.mark.parametrize("accumulate", [0, 1], ids=["store", "accumulate"])
def test_vecmat(lib, accumulate):
    """out[j] = sum_i v[i] W[i, j]: v[i] poisons every column, W[i, j] column j."""
    for rows, cols in nf.VECMAT:
        inp = on_device(nf.vecmat_inputs(rows, cols, accumulate))
        what = f"vecmat {rows}x{cols} acc={accumulate}"

        def run(d, poisoned):
            out, scratch = Guarded(1, cols, rup(cols, 8), torch.float32, prior=d["prior"]), Guarded(16, cols, cols, torch.float32)
            ok(lib.sgl_op_vecmat(P(d["v"]), P(d["W"]), rows, cols, scratch.ptr, 16 * cols * 4, out.ptr, accumulate, stream()))
            torch.cuda.synchronize()
            scratch.check(what + " scratch", written=not poisoned)
            return dict(out=checked(dict(out=out), what, poisoned)["out"][0])
        nf.drive(what, run, nf.vecmat_ref, inp, nf.vecmat_sites(rows, cols))


# =========================================================================================================
@pytest.mark.parametrize("accumulate", [0, 1], ids=["store", "accumulate"])
@pytest.mark.parametrize("dtype", nf.SUM_DTYPES, ids=lambda d: kr.DT_NAME[d])
def test_colsum(lib, dtype, accumulate):
    """x[i, j] poisons column j of the sum, whichever row chunk or column block holds it; ld > N with NaN in the slack."""
    for M, N in nf.COLSUM_SHAPES:
        inp = on_device(nf.colsum_inputs(dtype, M, N, accumulate))
        what = f"colsum {kr.DT_NAME[dtype]} {M}x{N} acc={accumulate}"

        def run(d, poisoned):
            out = Guarded(1, N, N, torch.float32, prior=d["prior"])
            chunks = max(1, min(256, (M + 511) // 512))
            scratch = torch.empty(chunks * N, device=DEV)
            ok(lib.sgl_op_colsum(dtype, P(padded(d["x"], N + 8)), N + 8, M, N, out.ptr, accumulate, P(scratch),
                                 scratch.numel() * 4, stream()))
            torch.cuda.synchronize()
            return dict(out=checked(dict(out=out), what, poisoned)["out"][0])
        nf.drive(what, run, nf.colsum_ref, inp, nf.colsum_sites(M, N))


@pytest.mark.parametrize("accumulate", [0, 1], ids=["store", "accumulate"])
def test_batch_sum(lib, accumulate):
    for B, n in nf.BATCH_SUM:
        inp = on_device(nf.batch_sum_inputs(B, n, accumulate))
        what = f"batch_sum {B}x{n} acc={accumulate}"

        def run(d, poisoned):
            out = Guarded(1, n, rup(n, 8), torch.float32, prior=d["prior"])
            ok(lib.sgl_op_batch_sum(P(d["x"]), B, n, out.ptr, accumulate, stream()))
            torch.cuda.synchronize()
            return dict(out=checked(dict(out=out), what, poisoned)["out"][0])
        nf.drive(what, run, nf.colsum_ref, inp, nf.batch_sum_sites(B, n))


@pytest.mark.parametrize("with_b", [0, 1], ids=["copy", "add"])
def test_add_f32(lib, with_b):
    """The copy keeps the class exactly (it keeps the bits); the sum is non-finite where either operand is."""
    for n in nf.ADD_N:
        inp = on_device(nf.add_inputs(n, with_b))
        what = f"{'add' if with_b else 'copy'}_f32 n={n}"

        def run(d, poisoned):
            out = Guarded(1, n, rup(n, 8), torch.float32)
            ok(lib.sgl_op_add_f32(P(d["a"]), P(d["b"]), out.ptr, n, stream()))
            torch.cuda.synchronize()
            got = checked(dict(out=out), what, poisoned)["out"][0]
            if not with_b:
                assert bool((nf.bits(got) == nf.bits(d["a"])).all()), f"{what}: the copy changed bits"
            return dict(out=got)
        nf.drive(what, run, nf.add_ref, inp, nf.add_sites(n, with_b))


@pytest.mark.parametrize("b_side,stacked", [(0, 0), (1, 1)], ids=["a_side_rows", "b_side_stack"])
def test_split3_parts_sum_to_nonfinite(lib, b_side, stacked):
    """The bf16x3 operand split: hi = bf16(x), lo = bf16(x - hi).  For x = +-inf, hi is inf and lo is inf - inf = NaN: the
    parts must SUM to a non-finite value, which is what the three MFMA products of the split GEMM add up; the two copies
    of hi are the same bits and the columns C..Cs stay zero."""
    R = nf.SPLIT3_R
    for C in nf.SPLIT3_C:
        Cs = rup(C, 8)
        inp = on_device(nf.split3_inputs(C))
        what = f"split3 C={C} b_side={b_side} stacked={stacked}"

        def run(d, poisoned):
            out = Guarded(3 * R, Cs, Cs, torch.bfloat16) if stacked else Guarded(R, 3 * Cs, 3 * Cs, torch.bfloat16)
            ld = rup(C, 4) + 4
            ok(lib.sgl_op_split3(P(padded(d["x"], ld)), R, C, ld, out.ptr, Cs, b_side, stacked, stream()))
            torch.cuda.synchronize()
            got = checked(dict(out=out), what, poisoned)["out"]
            seg = got.view(3, R, Cs) if stacked else got.view(R, 3, Cs).permute(1, 0, 2)
            hi, lo, hi2 = (seg[0], seg[1], seg[2]) if b_side else (seg[0], seg[2], seg[1])
            assert bool((nf.bits(hi) == nf.bits(hi2)).all()), f"{what}: the two hi parts differ"
            assert bool((seg[..., C:] == 0).all()), f"{what}: pad columns must be zero"
            return dict(sum=(hi.double() + lo.double())[:, :C])
        nf.drive(what, run, nf.split3_ref, inp, nf.split3_sites(C))


# =========================================================================================================
# attention probabilities, recomputed from q, k and the saved lse
# =========================================================================================================
@pytest.mark.parametrize("N,dh", nf.ATTN_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("dtype", nf.ATTN_DTYPES, ids=lambda d: kr.DT_NAME[d])
def test_attn_probs_full_and_head_mean(hiplib, dtype, N, dh):
    """sgl_op_attn_probs, FULL and HEAD_MEAN from the same poisoned operands: a q element poisons its query row, a k
    element its key column, an lse element its query row, in head (1, 0) of FULL and in image 1 of HEAD_MEAN; image 0 and
    the other head keep their bits.  The runner is tests/test_attn_maps_gpu.py's (guarded arenas, inputs verified const)."""
    from test_attn_maps_gpu import OpRun
    inp = nf.probs_inputs(dtype, N, dh)

    def run(d, poisoned):
        r = OpRun(hiplib, (nf.ATTN_B, nf.ATTN_H, N, dh), dtype, d["q"], d["k"], d["lse"])
        return dict(full=r.run(0)[0], head_mean=r.run(1)[0])
    nf.drive(f"attn_probs {kr.DT_NAME[dtype]} N={N} dh={dh}", run, nf.probs_ref, inp, nf.probs_sites(inp))


# =========================================================================================================
# fixed-order folds
# =========================================================================================================
@pytest.mark.parametrize("accumulate", [0, 1], ids=["store", "accumulate"])
def test_reduce_partials_and_splits(lib, accumulate):
    """reduce_partials (9 row blocks x 33 columns), reduce_partials3 (25 x 3 x 33: a column group that spans two outputs)
    and reduce_splits (5 slabs of 65 x 132): a partial poisons its column of its output and nothing else."""
    n, nblk = nf.RP_N, nf.RP_NBLK
    inp = on_device(nf.fold_inputs(nblk, n, accumulate, (n,)))

    def run1(d, poisoned):
        out = Guarded(1, n, rup(n, 8), torch.float32, prior=d["prior"])
        ok(lib.sgl_op_reduce_partials(P(padded(d["part"], n + 3)), nblk, n + 3, out.ptr, n, accumulate, stream()))
        torch.cuda.synchronize()
        return dict(out=checked(dict(out=out), "reduce_partials", poisoned)["out"][0])
    nf.drive(f"reduce_partials acc={accumulate}", run1, nf.fold_ref((n,)), inp, nf.fold_sites(nblk, n))

    n, nblk = nf.RP3_N, nf.RP3_NBLK
    inp = on_device(nf.fold_inputs(nblk, 3 * n, accumulate, (3, n)))

    def run3(d, poisoned):
        outs = [Guarded(1, n, rup(n, 8), torch.float32, prior=None if d["prior"] is None else d["prior"][k]) for k in range(3)]
        ok(lib.sgl_op_reduce_partials3(P(padded(d["part"], 3 * n + 5)), nblk, 3 * n + 5, outs[0].ptr, outs[1].ptr, outs[2].ptr,
                                       n, accumulate, accumulate, accumulate, stream()))
        torch.cuda.synchronize()
        got = checked({str(k): o for k, o in enumerate(outs)}, "reduce_partials3", poisoned)
        return dict(out=torch.cat([got[str(k)] for k in range(3)], 0))
    nf.drive(f"reduce_partials3 acc={accumulate}", run3, nf.fold_ref((3, n)), inp, nf.fold_sites(nblk, 3 * n))

    (N1, N2), splits = nf.RS_SHAPE, nf.RS_SPLITS
    inp = on_device(nf.fold_inputs(splits, N1 * N2, accumulate, (N1, N2)))

    def runs(d, poisoned):
        out = Guarded(N1, N2, N2 + 4, torch.float32, prior=d["prior"])
        ok(lib.sgl_op_reduce_splits(P(padded(d["part"], N1 * N2 + 8)), splits, N1 * N2 + 8, N1, N2, out.ptr, N2 + 4, accumulate,
                                    stream()))
        torch.cuda.synchronize()
        return checked(dict(out=out), "reduce_splits", poisoned)
    nf.drive(f"reduce_splits acc={accumulate}", runs, nf.fold_ref((N1, N2)), inp, nf.fold_sites(splits, N1 * N2))


# =========================================================================================================
# weight-shadow casts
# =========================================================================================================
def assert_class_kept(src, dst, what):
    """NaN -> NaN and +-inf -> +-inf of the same sign at every non-finite source element (dst indexed like src)."""
    for idx in (~torch.isfinite(src)).nonzero().tolist():
        v, g = src[tuple(idx)].item(), dst[tuple(idx)].float().item()
        assert (g != g) if v != v else (g == v), f"{what}: {v} became {g} at {idx}"


@pytest.mark.parametrize("dtype", nf.CAST_DTYPES, ids=lambda d: kr.DT_NAME[d])
def test_cast_pad_and_cast_job_keep_the_class(pkg, lib, dtype):
    """sgl_op_cast_pad (1 x 3 and 65 x 65 into a larger padded matrix) and a sgl_op_cast_job of one matrix with both
    destinations and one vector: the poisoned element arrives with its class exactly (NaN -> NaN, +-inf -> +-inf) in the
    destination, in the transposed destination and in the vector copy; every other element and the zero padding keep
    their bits."""
    tdt = tdt_of(dtype)
    for R, C in nf.CAST_PAD_SHAPES:
        Rp, Cp, lds = R + 5, C + 3, C + 1 + (C % 4 == 3)
        inp = on_device(nf.cast_pad_inputs(R, C))
        what = f"cast_pad {kr.DT_NAME[dtype]} {R}x{C}"

        def run(d, poisoned):
            dst = Guarded(Rp, Cp, Cp + 5, tdt)
            ok(lib.sgl_op_cast_pad(P(padded(d["src"], lds)), R, C, lds, dst.ptr, dtype, Rp, Cp, Cp + 5, stream()))
            torch.cuda.synchronize()
            got = checked(dict(dst=dst), what, poisoned)["dst"]
            assert_class_kept(d["src"], got, what)
            return dict(dst=got)
        nf.drive(what, run, nf.cast_pad_ref(Rp, Cp), inp, nf.mat_sites("src", R, C))
    j = nf.CAST_JOB
    inp = on_device(nf.cast_job_inputs())
    what = f"cast_job {kr.DT_NAME[dtype]}"

    def run_job(d, poisoned):
        L = pkg.lib
        src = padded(d["mat"], j["lds"])
        dst, dst_t = Guarded(j["Rp"], j["Cp"], j["ldd"], tdt), Guarded(j["Cp"], j["Rp"], j["ldt"], tdt)
        vec = Guarded(1, j["np"], rup(j["np"], 8), torch.float32)
        m = (L.SglCastMat * 1)(L.SglCastMat(P(src), dst.ptr, dst_t.ptr, j["R"], j["C"], j["lds"], j["Rp"], j["Cp"], j["ldd"],
                                            j["ldt"]))
        v = (L.SglCastVec * 1)(L.SglCastVec(P(d["vec"]), vec.ptr, j["n"], j["np"]))
        ok(lib.sgl_op_cast_job(m, 1, v, 1, dtype, stream()))
        torch.cuda.synchronize()
        got = checked(dict(dst=dst, dst_t=dst_t, vec=vec), what, poisoned)
        assert_class_kept(d["mat"], got["dst"], what + " dst")
        assert_class_kept(d["mat"], got["dst_t"].t(), what + " dst_t")
        assert_class_kept(d["vec"], got["vec"][0], what + " vec")
        return dict(dst=got["dst"], dst_t=got["dst_t"], vec=got["vec"][0])
    nf.drive(what, run_job, nf.cast_job_ref, inp, nf.cast_job_sites())


# =========================================================================================================
# patch gather / scatter and the position-table resize
# =========================================================================================================
@pytest.mark.parametrize("case", nf.IM2COL, ids=str)
@pytest.mark.parametrize("dtype", nf.CAST_DTYPES, ids=lambda d: kr.DT_NAME[d])
def test_im2col_col2im(lib, dtype, case):
    """im2col carries every covered pixel into exactly one element of the patch operand (all three output dtypes, the
    class kept), col2im every patch-gradient element back to exactly one pixel (fp32; the pad columns K..Kp hold NaN and
    are never read, the uncovered border stays +0)."""
    B, H, W, Pp, cl = case
    tdt = tdt_of(dtype)
    K, gh, gw = 3 * Pp * Pp, H // Pp, W // Pp
    Kp = rup(K, 64)
    inp = on_device(nf.im2col_inputs(B, H, W, Pp))
    what = f"im2col {kr.DT_NAME[dtype]} {case}"

    def run(d, poisoned):
        out = Guarded(B * gh * gw, Kp, Kp, tdt)
        src = d["pix"].contiguous(memory_format=torch.channels_last) if cl else d["pix"]
        ok(lib.sgl_op_im2col(P(src), cl, out.ptr, dtype, B, H, W, Pp, Kp, stream()))
        torch.cuda.synchronize()
        got = checked(dict(cols=out), what, poisoned)["cols"]
        bad = ~torch.isfinite(d["pix"])
        if poisoned:
            v, g = d["pix"][bad][0].item(), got[~torch.isfinite(got.float())].float()
            assert g.numel() == 1 and ((g[0] != g[0]) if v != v else (g[0] == v)), f"{what}: {v} arrived as {g.tolist()}"
        return dict(cols=got)
    nf.drive(what, run, nf.im2col_ref(Pp, Kp), inp, nf.im2col_sites(B, H, W, Pp))
    if dtype != kr.F32:
        return
    what = f"col2im {case}"

    def run_back(d, poisoned):
        out = Guarded(B * H * W, 3, 3, torch.float32) if cl else Guarded(B * 3 * H, W, W, torch.float32)
        ok(lib.sgl_op_col2im(P(padded(d["cols"], Kp)), B, H, W, Pp, Kp, out.ptr, cl, stream()))
        torch.cuda.synchronize()
        got = checked(dict(d_pixels=out), what, poisoned)["d_pixels"]
        return dict(d_pixels=got.view(B, H, W, 3).permute(0, 3, 1, 2) if cl else got.view(B, 3, H, W))
    nf.drive(what, run_back, nf.col2im_ref(H, W, Pp), inp, nf.col2im_sites(B, H, W, Pp))


@pytest.mark.parametrize("grid", nf.POS_GRIDS, ids=str)
def test_pos_resize_fwd_bwd(lib, grid):
    """The bicubic resize of the position table and its transpose (which ADDS onto a prior): a table element reaches the
    outputs whose sixteen taps read it, in its channel; an output-gradient element at most sixteen table entries."""
    g0, gh, gw = grid
    D = nf.POS_D
    inp = on_device(nf.pos_inputs(*grid))

    def run(d, poisoned):
        out = Guarded(gh * gw, D, D, torch.float32)
        ok(lib.sgl_op_pos_resize(P(d["table"]), g0, out.ptr, gh, gw, D, stream()))
        torch.cuda.synchronize()
        return checked(dict(out=out), f"pos_resize {grid}", poisoned)
    nf.drive(f"pos_resize {grid}", run, nf.pos_fwd_ref(*grid), inp, nf.mat_sites("table", g0 * g0, D))

    def run_back(d, poisoned):
        dt_ = Guarded(g0 * g0, D, D, torch.float32, prior=d["prior"])
        ok(lib.sgl_op_pos_resize_bwd(P(d["dout"]), gh, gw, dt_.ptr, g0, D, stream()))
        torch.cuda.synchronize()
        return checked(dict(dtable=dt_), f"pos_resize_bwd {grid}", poisoned)
    nf.drive(f"pos_resize_bwd {grid}", run_back, nf.pos_bwd_ref(*grid), inp, nf.mat_sites("dout", gh * gw, D), to_ref=on_host)


# =========================================================================================================
# cast
# =========================================================================================================
@pytest.mark.parametrize("dtype", nf.CAST_DTYPES, ids=lambda d: kr.DT_NAME[d])
def test_cast_f32_keeps_the_class(lib, dtype):
    """sgl_op_cast_f32 at the first element, the last one (in the 3-element tail) and the first of the tail: beyond the
    two rules the class is kept exactly, NaN -> NaN and +-inf -> +-inf of the same sign, in all three destination types."""
    tdt = tdt_of(dtype)
    n = nf.CAST_N
    inp = on_device(nf.cast_inputs())

    def run(d, poisoned):
        out = Guarded(1, n, n, tdt)
        ok(lib.sgl_op_cast_f32(P(d["src"]), out.ptr, dtype, n, stream()))
        torch.cuda.synchronize()
        dst = checked(dict(dst=out), f"cast_f32 {kr.DT_NAME[dtype]}", poisoned)["dst"][0]
        if poisoned:
            i = int((~torch.isfinite(d["src"])).nonzero()[0])
            v, g = d["src"][i].item(), dst[i].float().item()
            assert (g != g) if v != v else (g == v), f"cast_f32 {kr.DT_NAME[dtype]}: {v} became {g} at {i}"
        return dict(dst=dst)
    nf.drive(f"cast_f32 {kr.DT_NAME[dtype]}", run, nf.cast_ref, inp, nf.cast_sites())


# =========================================================================================================
# whole model: one corrupt image in a batch, one non-finite upstream gradient, and the skipped step
# =========================================================================================================
MODEL_MODES = [("fp32", False), ("bf16x3", False), ("bf16", False), ("fp16", False), ("bf16", True)]
MODE_IDS = [m + ("_recompute" if r else "") for m, r in MODEL_MODES]


@pytest.fixture(scope="module")
def tiny(pkg, oracle):
    """Config `tiny`, B = 2, seeded weights and pixels as in tests/test_optimizer_gpu.py; the CPU oracle's outputs and
    gradients per case, computed once and shared by the modes (never modified)."""
    cfg = pkg.get_config("tiny")
    sd = pkg.weights.seeded_state_dict(cfg, seed=3)
    x = pkg.weights.seeded_pixels(2, cfg.image_size, cfg.image_size, seed=4)
    x_nan = x.clone()
    x_nan[1, 1, cfg.image_size // 2, cfg.image_size // 2 + 1] = nf.NAN
    N = (cfg.image_size // cfg.patch_size) ** 2
    g = torch.Generator().manual_seed(9)
    ups = {}
    for name in ("pooler", "last_hidden"):
        gp = nf.nonzero(torch.randn(2, cfg.hidden_size, generator=g) * 0.01)
        gl = nf.nonzero(torch.randn(2, N, cfg.hidden_size, generator=g) * 0.01)
        if name == "pooler":
            gp[1, 5] = nf.INF
        else:
            gl[1, N - 1, cfg.hidden_size - 1] = nf.INF
        ups[name] = (gp, gl)
    cache = {}

    def oracle_grads(key):
        """key "pixel": the both-image loss on the NaN pixel; "pooler" / "last_hidden": the planted upstream gradient."""
        if key not in cache:
            ref = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
            out = oracle.vision_forward(x_nan if key == "pixel" else x, ref, cfg, True, False)
            if key == "pixel":
                both_image_loss(out["pooler_output"], out["last_hidden_state"]).backward()
            else:
                torch.autograd.backward([out["pooler_output"], out["last_hidden_state"]], list(ups[key]))
            cache[key] = (out, {k: v.grad for k, v in ref.items()})
        return cache[key]
    return dict(cfg=cfg, sd=sd, x=x, x_nan=x_nan, ups=ups, oracle_grads=oracle_grads)


def both_image_loss(pooled, last):
    return pooled.float().square().sum() + last.float().square().mean()


def make_model(pkg, tiny, mode, recompute=False):
    m = pkg.SiglipVisionModelHIP(tiny["cfg"], compute_dtype=mode, recompute=recompute)
    m.load_state_dict(tiny["sd"])
    return m.cuda()


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool((nf.bits(a.detach()) == nf.bits(b.detach())).all())


def assert_oracle_nonfinite_grads_arrive(model, ref_grads, what):
    """Rule 1 on the parameter gradients: every element the oracle makes non-finite is non-finite.  Returns how many
    parameters the oracle poisons."""
    hit = 0
    for n, p in model.named_parameters():
        r = ref_grads[n]
        if r is None or not bool(nf.nonfinite(r).any()):
            continue
        hit += 1
        assert p.grad is not None, f"{what}: {n} has no gradient"
        swallowed = nf.nonfinite(r) & torch.isfinite(p.grad.detach().cpu().double())
        if bool(swallowed.any()):
            i, idx = nf.first_index(swallowed)
            raise AssertionError(f"{what}: rule 1 (no swallowing): {n}.grad has {int(swallowed.sum())} finite elements "
                                 f"where the oracle's are not; first at {idx}: {p.grad.flatten()[i].item():.9g} "
                                 f"(bits {nf.hex_of(p.grad.detach(), i)})")
    return hit


@pytest.mark.parametrize("mode,recompute", MODEL_MODES, ids=MODE_IDS)
def test_model_one_corrupt_image(pkg, hiplib, tiny, mode, recompute):
    """A NaN in one pixel of image 1: image 0's last_hidden_state and pooler_output keep the bits of the clean forward,
    image 1's pooler_output is non-finite throughout, and after the backward of a loss over both images every
    parameter-gradient element the CPU oracle makes non-finite is non-finite (the oracle poisons every parameter: one
    corrupt image makes the step skip).  With requires_grad pixels, image 0's pixel gradient keeps the bits of the clean
    B = 2 run."""
    model = make_model(pkg, tiny, mode, recompute)
    what = f"model {mode}{' recompute' if recompute else ''} NaN pixel"
    ref_out, ref_grads = tiny["oracle_grads"]("pixel")
    assert bool(nf.nonfinite(ref_out["pooler_output"][1]).all()) and bool(torch.isfinite(ref_out["pooler_output"][0]).all())
    assert bool(torch.isfinite(ref_out["last_hidden_state"][0]).all())

    def run(x, px_grad):
        model.zero_grad(set_to_none=True)
        xd = x.cuda().requires_grad_(px_grad)
        out = model(pixel_values=xd)
        both_image_loss(out.pooler_output, out.last_hidden_state).backward()
        torch.cuda.synchronize()
        return out.pooler_output.detach().clone(), out.last_hidden_state.detach().clone(), \
            (xd.grad.clone() if px_grad else None)
    for px_grad in (False, True):
        p0, l0, gx0 = run(tiny["x"], px_grad)
        assert bool(torch.isfinite(p0).all()) and bool(torch.isfinite(l0).all())
        p1, l1, gx1 = run(tiny["x_nan"], px_grad)
        assert same_bits(p1[0], p0[0]), f"{what}: rule 2: pooler_output of image 0 changed"
        assert same_bits(l1[0], l0[0]), f"{what}: rule 2: last_hidden_state of image 0 changed"
        assert bool(nf.nonfinite(p1[1]).all()), f"{what}: rule 1: pooler_output of image 1 has finite elements"
        hit = assert_oracle_nonfinite_grads_arrive(model, ref_grads, what)
        assert hit == len(list(model.parameters())), f"{what}: the oracle poisons {hit} parameters only"
        if px_grad:
            assert bool(torch.isfinite(gx0).all()) and bool((gx0[0] != 0).any())
            assert same_bits(gx1[0], gx0[0]), f"{what}: rule 2: the pixel gradient of image 0 changed"


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_model_k_bias_gradient_without_q_bias_gradient(pkg, hiplib, tiny, mode):
    """The k_proj bias gradient is zero in real arithmetic and written as 0 * (column sums of dQ); with the q_proj biases
    frozen those sums are formed for it alone.  NaN pixel: every k_proj bias gradient is non-finite as the oracle's is;
    clean pixels: exact +0, as with the q_proj biases trained."""
    model = make_model(pkg, tiny, mode)
    for layer in model.encoder.layers:
        layer.self_attn.q_proj.bias.requires_grad_(False)
    _, ref_grads = tiny["oracle_grads"]("pixel")
    for x, clean in ((tiny["x"], True), (tiny["x_nan"], False)):
        model.zero_grad(set_to_none=True)
        out = model(pixel_values=x.cuda())
        both_image_loss(out.pooler_output, out.last_hidden_state).backward()
        torch.cuda.synchronize()
        for i, layer in enumerate(model.encoder.layers):
            assert layer.self_attn.q_proj.bias.grad is None
            g = layer.self_attn.k_proj.bias.grad
            if clean:
                assert bool((nf.bits(g) == 0).all()), f"layer {i}: the clean k_proj bias gradient is not +0"
            else:
                assert bool(nf.nonfinite(ref_grads[f"encoder.layers.{i}.self_attn.k_proj.bias"]).all())
                assert bool(nf.nonfinite(g).all()), f"layer {i}: rule 1: the k_proj bias gradient stayed finite"
        if not clean:
            frozen = {f"encoder.layers.{i}.self_attn.q_proj.bias" for i in range(len(model.encoder.layers))}
            for n, p in model.named_parameters():
                if n not in frozen:
                    assert bool(nf.nonfinite(p.grad).all()), f"{n}: rule 1"


@pytest.mark.parametrize("where", ["pooler", "last_hidden"])
@pytest.mark.parametrize("mode,recompute", MODEL_MODES, ids=MODE_IDS)
def test_model_inf_upstream_gradient_skips_the_step(pkg, hiplib, tiny, mode, recompute, where):
    """A clean forward with +inf in one element of the upstream gradient of pooler_output[1] (or of last_hidden_state[1]
    at the last token): every parameter-gradient element the oracle makes non-finite is non-finite, and
    siglip_amd.GradScaler + FusedAdamW (attach_encoder) skip the step: weights, moments and weight shadows keep their
    bits, the scale halves, and the next forward is bit-equal.  One clean step goes first, so that the moments exist and
    the shadows are the optimizer's."""
    model = make_model(pkg, tiny, mode, recompute)
    what = f"model {mode}{' recompute' if recompute else ''} +inf in d {where}"
    x = tiny["x"].cuda()
    gp, gl = (t.cuda() for t in tiny["ups"][where])
    clean_gp, clean_gl = (torch.where(torch.isfinite(t), t, torch.full_like(t, 0.01)) for t in (gp, gl))
    params = list(model.parameters())
    opt = pkg.FusedAdamW(params, lr=1e-3, weight_decay=0.05, max_grad_norm=1.0).attach_encoder(model)
    scale0 = 2.0 ** 8
    scaler = pkg.GradScaler("cuda", init_scale=scale0, growth_interval=1000)

    def step(a, b):
        out = model(pixel_values=x)
        loss = (out.pooler_output.float() * a).sum() + (out.last_hidden_state.float() * b).sum()
        opt.zero_grad(set_to_none=True)
        scaler.scale(loss).backward()
        grads_checked = None
        if a is gp:
            grads_checked = assert_oracle_nonfinite_grads_arrive(model, tiny["oracle_grads"](where)[1], what)
        scaler.step(opt)
        scaler.update()
        return grads_checked

    def snapshot():
        s = {f"p:{n}": p.detach().clone() for n, p in model.named_parameters()}
        for i, p in enumerate(params):
            for k in ("exp_avg", "exp_avg_sq"):      # `step` counts calls on the host; the device counts the skipped ones
                s[f"state{i}:{k}"] = opt.state[p][k].detach().clone()
        if model._shadows.arena is not None:
            s["shadows"] = model._shadows.arena.clone()
        with torch.no_grad():
            o = model(pixel_values=x)
            s["fwd:pooler"], s["fwd:last"] = o.pooler_output.clone(), o.last_hidden_state.clone()
        return s
    start = {n: p.detach().clone() for n, p in model.named_parameters()}
    step(clean_gp, clean_gl)
    assert scaler.get_scale() == scale0, f"{what}: the clean step was skipped"
    assert any(not same_bits(p, start[n]) for n, p in model.named_parameters()), "the clean step moved nothing"
    before = snapshot()
    assert len(before) > 3 * len(params)
    hit = step(gp, gl)
    assert hit > 0
    assert scaler.get_scale() == scale0 / 2, f"{what}: the scale did not halve: the overflow was not found"
    after = snapshot()
    assert sorted(after) == sorted(before)
    for k in before:
        assert same_bits(after[k], before[k]), f"{what}: {k} changed in a step that had to be skipped"


def test_model_mxfp8_one_corrupt_image(pkg, hiplib, tiny):
    """MX-fp8 inference with the NaN pixel: image 0 keeps its bits, image 1's outputs are non-finite (a non-finite row
    quantises to scale byte 0xFF and NaN elements, which the block-scaled GEMM turns into NaN)."""
    model = make_model(pkg, tiny, "mxfp8")
    with torch.no_grad():
        a = model(pixel_values=tiny["x"].cuda())
        p0, l0 = a.pooler_output.clone(), a.last_hidden_state.clone()
        b = model(pixel_values=tiny["x_nan"].cuda())
    assert bool(torch.isfinite(p0).all()) and bool(torch.isfinite(l0).all())
    assert same_bits(b.pooler_output[0], p0[0]) and same_bits(b.last_hidden_state[0], l0[0]), "image 0 changed"
    assert bool(nf.nonfinite(b.pooler_output[1]).all()), "pooler_output of image 1 has finite elements"
    assert bool(nf.nonfinite(b.last_hidden_state[1]).all()), "last_hidden_state of image 1 has finite elements"
