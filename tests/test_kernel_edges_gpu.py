"""GPU tests of the individual HIP kernels at the edges of their dispatch, through the C ABI (``sgl_op_*``).

Where tests/test_kernels_gpu.py compares one max/max number per tensor on friendly inputs, every check here is
element-wise against a float64 reference of the same operation on the same rounded inputs, with the bounds of
tests/kernel_ref.py (derived from the number formats, or carrying a constant set from a CPU emulation and asserted in
tests/test_kernel_ref_host.py).  No element is excused.  Outputs sit inside guard bands: rows before and after the tensor
and the columns between the logical width and the leading dimension hold a sentinel bit pattern that must come back
bit-identical, and the body is NaN-filled and must come back fully written.

Each parametrised case carries the name of the dispatch branch it is there for (dp48, dp96, ntile2, ln_fwd_multirow,
ln_bwd_multirow, nt256_scale, guard, posresize_rect, ...).
"""
import math

import pytest
import torch

import kernel_ref as kr
from attn_util import DEV, Guarded, P, check_attention, ok, rup, stream, tdt_of  # noqa: F401  (re-exported)
from kernel_ref import BF16, BF16X3, EPS32, F16, F32
from op_runners import gemm_nt, padded, run_gemm_nt, run_gemm_nt_qkv, run_gemm_tn, run_layernorm  # noqa: F401  (re-exported)

pytestmark = pytest.mark.gpu
LO = [BF16, F16]
ALL4 = [BF16, F16, F32, BF16X3]


@pytest.fixture(scope="module")
def lib(hiplib):
    assert torch.cuda.is_available()
    return hiplib


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def randn(g, *shape):
    return torch.randn(*shape, device=DEV, generator=g)


# =========================================================================================================
# GEMM NT
# =========================================================================================================
def nt_operands(dtype, M, N, K, seed):
    """A [M, K], B [N, K] in the operand dtype inside matrices whose leading dimension is 8 above K, NaN in the slack."""
    g = gen(seed)
    tdt = tdt_of(dtype)
    A = padded(randn(g, M, K).to(tdt), K + 8)
    B = padded((randn(g, N, K) / math.sqrt(K)).to(tdt), K + 8)
    bias = randn(g, N)
    return g, A, B, bias


def check_nt_epilogue(lib, dtype, M, N, K, epi, seed=0):
    """One NT GEMM launch with every leading dimension 8 above the logical width and guard bands round every output,
    checked in row chunks against the float64 reference (every row)."""
    g, A, B, bias = nt_operands(dtype, M, N, K, seed)
    tdt = tdt_of(dtype)
    f32_out = epi in (2, 5, 6)
    odt = torch.float32 if f32_out else tdt
    u, tiny = kr.UNIT[odt], kr.TINY[odt]
    res = aux = pos = None
    if epi == 2:
        res = padded(randn(g, M, N), N + 8)
    if epi == 4:
        aux = padded((randn(g, M, N) * 1.5).to(odt), N + 24)
    if epi == 5:
        pos = randn(g, 37, N)
    out, out2 = run_gemm_nt(lib, dtype, M, N, K, epi, A, B, None if epi == 4 else bias, res, aux, pos)
    what = f"NT {kr.DT_NAME[dtype]} M={M} N={N} K={K} epi={epi}"
    out.check(what)
    if out2 is not None:
        out2.check(what + " out2")
    Bk = B[:, :K]
    worst = 0.0
    step = 4096
    for r0 in range(0, M, step):
        r1 = min(M, r0 + step)
        Ak = A[r0:r1, :K]
        adds = []
        if epi != 4:
            adds.append(bias[None, :].expand(r1 - r0, N))
        if epi == 2:
            adds.append(res[r0:r1, :N])
        if epi == 5:
            adds.append(pos[torch.arange(r0, r1, device=DEV) % 37])
        ref, bound, accb = kr.gemm_ref(Ak, Bk, K, u, adds, tiny)
        got = out.got()[r0:r1]
        if epi == 4:
            uu = aux[r0:r1, :N]
            gp = kr.gelu_grad64(uu)
            t = kr.gelu_eval_term(uu[::16], grad=True)
            full = ref * gp
            worst = max(worst, kr.assert_within(got, full, u * full.abs() + tiny + gp.abs() * accb + ref.abs() * t,
                                                what))
            continue
        worst = max(worst, kr.assert_within(got, ref, bound, what))
        if epi == 1:
            t = kr.gelu_eval_term(ref[::16])
            act = kr.gelu64(ref)
            bact = u * act.abs() + tiny + kr.gelu_grad64(ref).abs() * accb + t
            worst = max(worst, kr.assert_within(out2.got()[r0:r1], act, bact, what + " gelu"))
        if epi in (0, 1) and odt != torch.float32 and (r1 - r0) * N >= 10000:
            kr.assert_rounding_unbiased(got, ref, u, what)
    return worst


NT_NK = [(384, 192), (264, 72), (1160, 200)]


NT_KERNELS = [(BF16, 333, "bf16_small_tile"), (BF16, 2333, "bf16_nt256"), (F16, 333, "f16_small_tile"),
              (F16, 2333, "f16_nt256"), (F32, 333, "f32_strict"), (F32, 2049, "f32_strict_m2049")]


@pytest.mark.parametrize("epi", [0, 1, 2, 4, 5, 6], ids=lambda e: f"epi{e}")
@pytest.mark.parametrize("N,K", NT_NK, ids=lambda v: str(v))
@pytest.mark.parametrize("dtype,M,name", NT_KERNELS, ids=lambda v: str(v))
def test_gemm_nt_epilogues_ld_guard(lib, dtype, M, name, N, K, epi):
    """Every epilogue on both kernel generations of the 16-bit GEMMs (M = 333: 128-row tiles; M = 2333: the 256x256 tile)
    and on the strict fp32 kernel (one generation; M = 333 and 2049), lda / ldb / ldo / ldo2 / ldr / ldaux all above the
    logical width, guard bands round the outputs.
    GELU evaluation term: 4 x the largest fp32-formula deviation over the case's own pre-activations, about 2e-6 for
    the activation and 8e-6 for the derivative (kernel_ref.gelu_eval_term)."""
    check_nt_epilogue(lib, dtype, M, N, K, epi, seed=M + N + epi)


@pytest.mark.parametrize("epi", [1, 4], ids=lambda e: f"epi{e}")
@pytest.mark.parametrize("gen_,M", [("small_tile", 333), ("nt256", 2333)], ids=lambda v: str(v))
@pytest.mark.parametrize("dtype", LO, ids=lambda d: kr.DT_NAME[d])
def test_gemm_nt_padded_mlp_width_guard(lib, dtype, gen_, M, epi):
    """The encoder's MLP width: 4304 logical columns in a wider buffer, fc1 + GELU and GELU backward."""
    check_nt_epilogue(lib, dtype, M, 4304, 1152, epi, seed=epi)


@pytest.mark.parametrize("M", [2047, 2048], ids=lambda v: f"M{v}")
@pytest.mark.parametrize("N", [248, 256], ids=lambda v: f"N{v}")
@pytest.mark.parametrize("dtype", LO, ids=lambda d: kr.DT_NAME[d])
def test_gemm_nt_dispatch_edge_guard(lib, dtype, M, N):
    """Both sides of the small-tile | 256-tile gate (M >= 2048 && N >= 256)."""
    check_nt_epilogue(lib, dtype, M, N, 72, 0, seed=M + N)
    check_nt_epilogue(lib, dtype, M, N, 72, 2, seed=M + N)


@pytest.mark.parametrize("K", [8, 40, 64, 72], ids=lambda v: f"K{v}")
@pytest.mark.parametrize("gen_,M", [("small_tile", 333), ("nt256", 2333)], ids=lambda v: str(v))
@pytest.mark.parametrize("dtype", LO, ids=lambda d: kr.DT_NAME[d])
def test_gemm_nt_k_steps_guard(lib, dtype, gen_, M, K):
    """K from under one K-step through exactly one to a tail."""
    check_nt_epilogue(lib, dtype, M, 264, K, 0, seed=K)


@pytest.mark.parametrize("name,N,epi", [("nt256_scale_res_f32", 1152, 2), ("nt256_scale_fc1_gelu_ld4352", 4304, 1)],
                         ids=lambda v: str(v))
def test_gemm_nt_production_scale(lib, name, N, epi):
    """The benchmark batch: M = 93312 rows, 365 row tiles of the 256x256 kernel (its tile_of_local order over 8 XCD ranges),
    EVERY row against the float64 reference in chunks of 4096 rows.  The fc1 case writes 4304 columns into rows of 4312
    with a guard band (the encoder's buffers are 4352 wide: same property, columns N..ld stay untouched)."""
    check_nt_epilogue(lib, BF16, 93312, N, 1152, epi, seed=7)
    torch.cuda.empty_cache()


@pytest.mark.parametrize("batch,tokens,heads,hd", [(2, 50, 12, 8), (7, 300, 12, 8), (2, 50, 4, 40), (7, 300, 4, 40),
                                                   (2, 50, 3, 96), (7, 300, 3, 96)],
                         ids=lambda v: str(v))
@pytest.mark.parametrize("dtype", [BF16, F16, F32], ids=lambda d: kr.DT_NAME[d])
def test_gemm_nt_qkv_scatter_guard(lib, dtype, batch, tokens, heads, hd):
    """EPI_QKV at head dims 8, 40 and 96 on both kernel generations (batch*tokens = 100 and 2100), guard band round the
    [3][B][H][N][hdp] tensor, pad columns written as zero."""
    g = gen(hd + batch)
    tdt = tdt_of(dtype)
    D = heads * hd
    hdp = rup(hd, 16)
    M, N, K = batch * tokens, 3 * D, D
    A = padded(randn(g, M, K).to(tdt), K + 8)
    B = padded((randn(g, N, K) / math.sqrt(K)).to(tdt), K + 8)
    bias = randn(g, N)
    out = run_gemm_nt_qkv(lib, dtype, A, B, bias, batch, tokens, heads, hd, hdp)
    what = f"QKV {kr.DT_NAME[dtype]} hd={hd} M={M}"
    out.check(what)
    ref, bound, _ = kr.gemm_ref(A[:, :K], B[:, :K], K, kr.UNIT[tdt], [bias[None, :].expand(M, N)], kr.TINY[tdt])
    perm = lambda t: t.view(batch, tokens, 3, heads, hd).permute(2, 0, 3, 1, 4)
    got = out.got().view(3, batch, heads, tokens, hdp)
    kr.assert_within(got[..., :hd], perm(ref), perm(bound), what)
    if hdp > hd:
        assert bool((got[..., hd:] == 0).all()), "pad columns must be written as zero"


# =========================================================================================================
# GEMM TN
# =========================================================================================================
def check_tn(lib, dtype, Mred, N1, N2, splits=1, accumulate=0, ws_bytes=None, seed=0):
    g = gen(seed)
    tdt = tdt_of(dtype)
    lda, ldb, ldo = rup(N1, 8) + 8, rup(N2, 8) + 8, rup(N2, 4) + 4
    rows = max(Mred, 1)
    A = padded(randn(g, rows, N1).to(tdt), lda)
    B = padded(randn(g, rows, N2).to(tdt), ldb)
    prior = randn(g, N1, N2) * 3 if accumulate else None
    out = run_gemm_tn(lib, dtype, A, B, Mred, N1, N2, ldo, splits, accumulate, prior, ws_bytes)
    what = f"TN {kr.DT_NAME[dtype]} Mred={Mred} N1={N1} N2={N2} acc={accumulate}"
    out.check(what)
    ref, bound = kr.gemm_tn_ref(A[:Mred, :N1], B[:Mred, :N2], Mred, prior)
    return kr.assert_within(out.got(), ref, bound, what)


@pytest.mark.parametrize("name,Mred,N1,N2", [("gate_mred_below", 2047, 512, 512), ("gate_tn256", 2048, 512, 512),
                                             ("gate_n1_below", 2048, 504, 512), ("gate_n2_below", 2048, 512, 504),
                                             ("mred_not_mult64", 333, 136, 72), ("tn256_mred_tail", 4133, 520, 1152)],
                         ids=lambda v: str(v))
@pytest.mark.parametrize("accumulate", [0, 1], ids=["store", "accumulate_onto_nonzero"])
@pytest.mark.parametrize("dtype", LO, ids=lambda d: kr.DT_NAME[d])
def test_gemm_tn_gate_ld_guard(lib, dtype, accumulate, name, Mred, N1, N2):
    """The 256-tile gate (N1 >= 512 && N2 >= 512 && Mred >= 2048) from both sides, ldo > N2 with a guard band, accumulate
    onto a non-zero matrix, reductions that are not a multiple of the K-step.  Split-K (the 256-tile launcher splits on its
    own) needs no term in the bound: see kernel_ref.gemm_tn_ref."""
    check_tn(lib, dtype, Mred, N1, N2, splits=3 if N1 < 512 else 1, accumulate=accumulate, seed=Mred + N1)


@pytest.mark.parametrize("accumulate", [0, 1], ids=["memset", "untouched"])
@pytest.mark.parametrize("dtype", [BF16, F16], ids=lambda d: kr.DT_NAME[d])
def test_gemm_tn_empty_reduction_guard(lib, dtype, accumulate):
    """Mred = 0: zeros without accumulate, the prior with it; nothing outside N1 x N2 either way."""
    check_tn(lib, dtype, 0, 136, 72, accumulate=accumulate, seed=1)


@pytest.mark.parametrize("name,N2,ws_bytes", [("ws_too_small_atomics", 512, 4096), ("ws_n2_mod4_atomics", 514, 64 << 20),
                                              ("ws_slabs", 512, 64 << 20)], ids=lambda v: str(v))
@pytest.mark.parametrize("accumulate", [0, 1], ids=["store", "accumulate"])
def test_gemm_tn_ws_fallbacks_guard(lib, name, N2, ws_bytes, accumulate):
    """sgl_op_gemm_tn_ws with scratch too small for the slabs and with N2 % 4 != 0: both fall back to fp32 atomics and
    must still be correct; the slab path for comparison."""
    check_tn(lib, BF16, 6000, 1152, N2, accumulate=accumulate, ws_bytes=ws_bytes, seed=N2)


# =========================================================================================================
# attention
# =========================================================================================================
DP_OF = {8: "dp16_chunk1", 24: "dp32_pad_chunk4", 40: "dp48_pad_chunk6", 48: "dp48", 56: "dp64_pad_chunk8", 88: "dp96_pad_chunk12",
         96: "dp96"}


@pytest.mark.parametrize("N", [65, 130], ids=lambda v: f"N{v}")
@pytest.mark.parametrize("dh", sorted(DP_OF), ids=lambda d: f"dh{d}_{DP_OF[d]}")
@pytest.mark.parametrize("layout", ["token", "head"])
@pytest.mark.parametrize("dtype", ALL4, ids=lambda d: kr.DT_NAME[d])
def test_attention_head_dims(lib, dtype, layout, dh, N):
    """Every DP instantiation (16, 32, 48, 64, 96; 80 is dh = 72 below) and every dh % 16 class, B*H = 3 (not a multiple
    of 8), forward and backward."""
    check_attention(lib, dtype, layout, "gauss", 1, 3, N, dh, seed=dh + N)


N_EDGES = [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 256, 257, 384]


def _n_id(N):
    return f"N{N}_ntile{(N + 63) // 64}_wg{(N + 127) // 128}"


@pytest.mark.parametrize("N", N_EDGES, ids=_n_id)
@pytest.mark.parametrize("dh,layout", [(72, "token"), (64, "head")], ids=["dh72_dp80_token", "dh64_dp64_head"])
@pytest.mark.parametrize("dtype", ALL4, ids=lambda d: kr.DT_NAME[d])
def test_attention_token_count_edges(lib, dtype, dh, layout, N):
    """The edges of the 32-query wave, the 64-key tile and the 128-row workgroup; ntiles 1 -> 2 -> 3 and on, where the
    two-stage forward ring and the three-stage backward ring wrap; multiples of 128 above 128."""
    check_attention(lib, dtype, layout, "gauss", 2, 2, N, dh, seed=N)


@pytest.mark.parametrize("N", [65, 130, 256], ids=_n_id)
@pytest.mark.parametrize("dtype", ALL4, ids=lambda d: kr.DT_NAME[d])
def test_attention_token_layout_exact_extent(lib, dtype, N):
    """Token layout with ld == 3 D exactly and nothing of the matrix behind its last row: NaN blocks lie directly before
    and after it in the same allocation, so the kernels' own extent is what keeps them in bounds."""
    check_attention(lib, dtype, "token", "gauss", 1, 3, N, 72, seed=N, exact_extent=True)


HOSTILE = [("jump_last_tile_first_half", "jump", 260), ("jump_last_tile_second_half", "jump", 290),
           ("jump_not_last_tile", "jump", 100), ("peaked_one_hot", "peaked", None), ("flat", "flat", None),
           ("offset60", "offset", None)]


@pytest.mark.parametrize("name,kind,jump_key", HOSTILE, ids=lambda v: str(v))
@pytest.mark.parametrize("layout", ["token", "head"])
@pytest.mark.parametrize("dtype", ALL4, ids=lambda d: kr.DT_NAME[d])
def test_attention_hostile_inputs_fwd_bwd(lib, dtype, layout, name, kind, jump_key):
    """N = 300 (five 64-key tiles, the last one 44 keys), dh = 64: a running max that jumps at a late tile (in either
    32-key half of the last tile, and in a tile that is not the last), a softmax that is one-hot to fp32 precision, a
    near-uniform one, and scores shifted by a common +60.  Inputs and |score * scale| stay inside fp16 range."""
    r, _ = check_attention(lib, dtype, layout, kind, 1, 2, 300, 64, seed=4, jump_key=jump_key)
    if kind == "jump":
        assert r["P"][0, :, 7, jump_key].min().item() > 0.999
    if kind == "peaked":
        assert (r["P"].max(-1).values > 1 - 2.0 ** -24).float().mean().item() > 0.8


@pytest.mark.parametrize("BH", [1, 7, 8, 9, 17], ids=lambda v: f"heads{v}_xcd_map")
@pytest.mark.parametrize("layout", ["token", "head"])
@pytest.mark.parametrize("dtype", LO, ids=lambda d: kr.DT_NAME[d])
def test_attention_head_block_mapping(lib, dtype, layout, BH):
    """B*H below, at and above the 8 XCDs, including counts that need padding heads in the head_block mapping."""
    B, H = (1, BH) if BH != 9 else (3, 3)
    check_attention(lib, dtype, layout, "gauss", B, H, 130, 72, seed=BH)


@pytest.mark.parametrize("layout", ["token", "head"])
@pytest.mark.parametrize("dtype", LO, ids=lambda d: kr.DT_NAME[d])
def test_attention_pack_rounding_unbiased(lib, dtype, layout):
    """With v, dout > 0 nothing cancels in P.V and P^T.dO, so a P pack (or output store) that truncates shows as a signed
    bias the element-wise bound cannot see (it is 3u |O| at its tightest, truncation errs by < 2u |O|):
    mean((got - ref) / (u ref)) within +-0.05 on O and on dV, the margin of the GEMM store statistic.  Round-to-nearest
    measures within +-0.01 in the CPU emulation, truncation below -0.7 (tests/test_kernel_ref_host.py)."""
    r, (O, dV) = check_attention(lib, dtype, layout, "positive", 1, 2, 300, 64, seed=9)
    u = kr.UNIT[tdt_of(dtype)]
    kr.assert_rounding_unbiased(O, r["O"], u, "attention O")
    kr.assert_rounding_unbiased(dV, r["dV"], u, "attention dV")


# =========================================================================================================
# LayerNorm
# =========================================================================================================
def check_layernorm(lib, x, odt_code, seed=0, dres=True, dgamma=True, dbeta=True, chunk=8192, bias_stat=False,
                    dy_code=None, lp_code=None):
    """sgl_op_layernorm_fwd then _bwd (from the forward's own statistics, as the encoder does) on x [M, D] fp32, every row
    against float64 in row chunks.  dy and the low-precision copy of dx are in the forward's output dtype unless given."""
    M, D = x.shape
    g = gen(seed)
    odt = tdt_of(odt_code)
    u = kr.UNIT[odt]
    gam, bet = randn(g, D) * 0.2 + 1, randn(g, D) * 0.1
    what = f"LayerNorm M={M} D={D} {kr.DT_NAME[odt_code]}"
    dy_code = odt_code if dy_code is None else dy_code
    lp_code = odt_code if lp_code is None else lp_code
    lpt = tdt_of(lp_code)
    dy = randn(g, M, D).to(tdt_of(dy_code))
    dr = randn(g, M, D) if dres else None
    o = run_layernorm(lib, x, gam, bet, dy, dr, odt_code, dy_code, lp_code, dgamma, dbeta)
    y, mean, rstd, dx, dxlp, dg, db = (o[n] for n in ("y", "mean", "rstd", "dx", "dx_lp", "dgamma", "dbeta"))
    for t, n in ((y, "y"), (mean, "mean"), (rstd, "rstd")):
        t.check(f"{what} {n}")
    mu_k, rs_k = mean.got()[0], rstd.got()[0]
    dx.check(what + " dx")
    dxlp.check(what + " dx_lp")
    dg_ref = torch.zeros(D, device=DEV, dtype=torch.float64)
    dg_mag, db_ref, db_mag = dg_ref.clone(), dg_ref.clone(), dg_ref.clone()
    for r0 in range(0, M, chunk):
        r1 = min(M, r0 + chunk)
        (yr, by), (mr, bm), (rr, br) = kr.ln_fwd_ref(x[r0:r1], gam, bet, 1e-6, u, tiny_out=kr.TINY[odt])
        kr.assert_within(y.got()[r0:r1], yr, by, f"{what} y rows {r0}..")
        kr.assert_within(mu_k[r0:r1], mr, bm, f"{what} mean rows {r0}..")
        kr.assert_within(rs_k[r0:r1], rr, br, f"{what} rstd rows {r0}..")
        if bias_stat and odt != torch.float32 and (r1 - r0) * D >= 10000:
            kr.assert_rounding_unbiased(y.got()[r0:r1], yr, u, what + " y")
        (dxr, b32, blp), (g_r, g_b), (b_r, b_b) = kr.ln_bwd_ref(dy[r0:r1], x[r0:r1], mu_k[r0:r1], rs_k[r0:r1], gam,
                                                                None if dr is None else dr[r0:r1],
                                                                kr.UNIT[lpt], tiny_out=kr.TINY[lpt])
        kr.assert_within(dx.got()[r0:r1], dxr, b32, f"{what} dx rows {r0}..")
        kr.assert_within(dxlp.got()[r0:r1], dxr, blp, f"{what} dx_lp rows {r0}..")
        k_chunk = ((r1 - r0) / 4 + 8) * EPS32                 # undo the chunk's own factor: the whole sum has M terms
        dg_ref += g_r
        dg_mag += g_b / k_chunk
        db_ref += b_r
        db_mag += b_b / k_chunk
    k_all = (M / 4 + 8) * EPS32
    if dg:
        dg.check(what + " dgamma")
        kr.assert_within(dg.got()[0], dg_ref, k_all * dg_mag, what + " dgamma")
    if db:
        db.check(what + " dbeta")
        kr.assert_within(db.got()[0], db_ref, k_all * db_mag, what + " dbeta")


LN_D = {4: "D4_one_float4", 64: "D64", 512: "D512_maxv2_last", 516: "D516_maxv5_first", 1152: "D1152",
        1280: "D1280_maxv5_last", 1284: "D1284_maxv8_first", 2048: "D2048_maxv8_last"}


@pytest.mark.parametrize("odt", [F32, BF16, F16], ids=lambda d: "out_" + kr.DT_NAME[d])
@pytest.mark.parametrize("D", sorted(LN_D), ids=lambda d: LN_D[d])
def test_layernorm_width_boundaries(lib, D, odt):
    """Both sides of each LN_MAXV instantiation (2 | 5 | 8 float4 per lane), the narrowest and the widest row."""
    check_layernorm(lib, randn(gen(D), 5, D) * 2 + 0.3, odt, seed=D)


@pytest.mark.parametrize("M", [1, 3, 4, 5, 3072, 3073], ids=lambda m: f"M{m}" + ("_ln_bwd_multirow" if m > 3072 else ""))
@pytest.mark.parametrize("D,odt", [(1152, BF16), (64, F16)], ids=["D1152_bf16", "D64_f16"])
def test_layernorm_row_counts(lib, D, odt, M):
    """Partial workgroups (4 rows each) and the backward's grid cap: 768 workgroups hold 3072 rows, row 3073 is the first
    that a wave reaches in its second trip."""
    check_layernorm(lib, randn(gen(M), M, D) * 2 + 0.3, odt, seed=M, bias_stat=M * D >= 10000)


@pytest.mark.parametrize("M", [65536, 65543], ids=lambda m: f"M{m}" + ("_ln_fwd_multirow" if m > 65536 else "_grid_cap"))
@pytest.mark.parametrize("D,odt", [(1152, BF16), (64, F32)], ids=["D1152_bf16", "D64_f32"])
def test_layernorm_multirow_loops(lib, D, odt, M):
    """ln_fwd_kernel caps its grid at 16384 workgroups = 65536 rows; above that each wave loops over rows with a one-row
    prefetch (the benchmark batch, M = 93312, runs in that loop all the time).  The backward loops from M = 3073 on.
    EVERY row is checked against the float64 reference, in chunks on the device."""
    x = randn(gen(M + D), M, D) * 2 + 0.3
    x += torch.arange(M, device=DEV, dtype=torch.float32)[:, None] % 7      # rows differ in mean: a wrong row is visible
    check_layernorm(lib, x, odt, seed=M, bias_stat=True)
    torch.cuda.empty_cache()


@pytest.mark.parametrize("family", ["gauss", "mean1000", "const_exact", "const_inexact", "outlier", "zeros"])
@pytest.mark.parametrize("odt", [F32, BF16, F16], ids=lambda d: "out_" + kr.DT_NAME[d])
def test_layernorm_input_families(lib, odt, family):
    """A row mean that dwarfs the spread (where a one-pass variance fails), constant rows (variance 0, rstd = 1000) with a
    row sum that is exact in fp32 (0.5) and one that is not (1000.1: the case the |mu| term of the bound exists for), one
    channel at 300x the rest, a row of zeros."""
    x = kr.ln_families(37, 1152, seed=3, device=DEV)[family]
    check_layernorm(lib, x, odt, seed=5, bias_stat=family in ("gauss", "outlier"))


@pytest.mark.parametrize("lp", [F32, BF16, F16], ids=lambda d: "lp_" + kr.DT_NAME[d])
@pytest.mark.parametrize("dy", [F32, BF16, F16], ids=lambda d: "dy_" + kr.DT_NAME[d])
@pytest.mark.parametrize("D", [64, 516, 1284], ids=["maxv2", "maxv5", "maxv8"])
def test_layernorm_bwd_dtype_pairs(lib, D, dy, lp):
    """ln_bwd_kernel is instantiated for every (dy dtype, dx_lp dtype, LN_MAXV) triple: 27 kernels, each launched once."""
    check_layernorm(lib, randn(gen(D + dy), 9, D) * 2 + 0.3, F32, seed=D, dy_code=dy, lp_code=lp)


@pytest.mark.parametrize("dres,dgamma,dbeta", [(False, True, True), (True, False, False), (False, False, True),
                                               (False, True, False)],
                         ids=["no_dres", "no_dgamma_dbeta", "dbeta_only", "dgamma_only"])
def test_layernorm_bwd_optional_outputs(lib, dres, dgamma, dbeta):
    check_layernorm(lib, randn(gen(8), 77, 516) * 2 + 0.3, BF16, seed=8, dres=dres, dgamma=dgamma, dbeta=dbeta)


# =========================================================================================================
# small ops
# =========================================================================================================
COLSUM_SHAPES = [(1, 8, "one_row"), (511, 256, "one_chunk_one_colblock"), (512, 264, "two_colblocks"),
                 (1000, 136, "two_chunks"), (93312, 1152, "bench_batch"), (131585, 72, "chunk_cap_256")]


@pytest.mark.parametrize("M,N,name", COLSUM_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("accumulate", [0, 1], ids=["store", "accumulate"])
@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=lambda d: kr.DT_NAME[d])
def test_colsum_dtypes_shapes_ld_guard(lib, dtype, accumulate, M, N, name):
    """Every input dtype, more than one column block (N > 256), the colsum_chunks cap (M > 131072), accumulate, and
    ld > N with NaN in the slack.  Bound (M/4 + 8) 2^-24 colsum|x|: any summation order of M fp32 terms."""
    g = gen(M + N)
    x = padded(randn(g, M, N).to(tdt_of(dtype)), N + 8)
    prior = randn(g, 1, N) * 5 if accumulate else None
    out = Guarded(1, N, N, torch.float32, prior=prior)
    chunks = max(1, min(256, (M + 511) // 512))
    scratch = torch.empty(chunks * N, device=DEV)
    ok(lib.sgl_op_colsum(dtype, P(x), N + 8, M, N, out.ptr, accumulate, P(scratch), scratch.numel() * 4, stream()))
    out.check("colsum")
    ref, bound = kr.colsum_ref(x[:, :N], M, None if prior is None else prior[0])
    kr.assert_within(out.got()[0], ref, bound, f"colsum {kr.DT_NAME[dtype]} {M}x{N}")


@pytest.mark.parametrize("g0,gh,gw", [(2, 3, 7), (3, 7, 3), (14, 16, 27), (27, 1, 5), (27, 16, 27), (14, 27, 16)],
                         ids=lambda v: str(v))
def test_posresize_rect(lib, g0, gh, gw):
    """Non-square targets (gh != gw in both orders, a single row) against float64 F.interpolate(bicubic,
    align_corners=False), without antialias as the HF path and oracle/siglip_oracle.py."""
    D = 40
    t = randn(gen(g0 * 100 + gh), g0 * g0, D)
    out = Guarded(gh * gw, D, D, torch.float32)
    ok(lib.sgl_op_pos_resize(P(t), g0, out.ptr, gh, gw, D, stream()))
    out.check("pos_resize")
    ref = kr.pos_resize_ref(t, g0, gh, gw)
    bound = kr.pos_resize_bound(t, g0)[None, :].expand_as(ref)
    kr.assert_within(out.got(), ref, bound, f"posresize_rect {g0}->{gh}x{gw}")


@pytest.mark.parametrize("Bn,Hh,Ww,Pp,cl,name", [(2, 42, 28, 14, 0, "w_ne_h"), (1, 45, 42, 14, 0, "remainder_h_only"),
                                                 (1, 42, 45, 14, 1, "remainder_w_only_nhwc"),
                                                 (2, 32, 48, 16, 1, "w_ne_h_nhwc")], ids=lambda v: str(v))
@pytest.mark.parametrize("odt", [F32, BF16, F16], ids=lambda d: "out_" + kr.DT_NAME[d])
def test_im2col_dtypes_rect_guard(lib, odt, Bn, Hh, Ww, Pp, cl, name):
    """bf16 / fp16 outputs equal the fp32 gather rounded to nearest, bit for bit; W != H; a remainder in one dimension."""
    pix = randn(gen(Hh + Ww), Bn, 3, Hh, Ww)
    K = 3 * Pp * Pp
    Kp = rup(K, 64)
    gh, gw = Hh // Pp, Ww // Pp
    out = Guarded(Bn * gh * gw, Kp, Kp, tdt_of(odt))
    src = pix.contiguous(memory_format=torch.channels_last) if cl else pix
    ok(lib.sgl_op_im2col(P(src), cl, out.ptr, odt, Bn, Hh, Ww, Pp, Kp, stream()))
    out.check("im2col")
    ref = torch.nn.functional.unfold(pix[:, :, :gh * Pp, :gw * Pp], Pp, stride=Pp).transpose(1, 2).reshape(-1, K)
    assert torch.equal(out.got()[:, :K], ref.to(tdt_of(odt)))
    assert bool((out.got()[:, K:] == 0).all())
