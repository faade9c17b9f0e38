"""GPU: single-kernel launches through the C ABI whose operands or outputs cross 2^31 bytes, 2^32 bytes or 2^31 elements,
checked exactly.

NT GEMM "row stamps".  The operands are small integers chosen so that every output element is an integer that its output
type represents exactly and that its (row, column) determines; the expected tensor is rebuilt on the device from
coordinates alone and compared over ALL elements, guard rows and the slack between width and leading dimension included.
A[m, i] = bits 2i, 2i + 1 of m (i < 12, so 24 bits: every m below 2^24), A[m, 12] = 1, zero elsewhere.  Row j of B holds one
scale s_j at column j % 12 and one base c_j at column 12, so acc[m, j] = s_j * field(m, j % 12) + c_j: the twelve fields
together name the row (two distinct rows never share a stamp), and c_j names the column (two distinct columns never share a
value within a row).  fp16 (11-bit significand): s_j = 1, c_j = 4 j, values up to 2047.  bf16 (8-bit significand):
s_j = 2^(j >> 5), c_j = s_j (128 + 4 (j & 31)): the significand holds the low five column bits and the field, the exponent
the rest.  All sums stay below 2^24, so fp32 accumulation is exact in any order.

M = 493 447 rows of lda = 4352 put the A operand 0.1 % under the GEMMs' 2^32-byte guard; output leading dimensions are
chosen so that the output crosses 2^32 bytes (4352 for fp32 outputs, 8704 for 16-bit ones).

A test skips only when torch.cuda.mem_get_info() shows less free memory than the bytes it is about to allocate."""
import os
import subprocess
import sys
import time

import pytest
import torch

import attn_grad_ref as agr
import attn_probs_ref as apr
import kernel_ref as kr
from attn_util import DEV, Guarded, P, ok, stream, tdt_of
from kernel_ref import BF16, F16, F32
from op_runners import gemm_nt, run_gemm_tn

pytestmark = pytest.mark.gpu

M_NT, LDA = 493_447, 4352
ERR_UNSUPPORTED = -2     # how the single-kernel entry points report a launcher's refusal (hipErrorInvalidValue)
STORE, BIAS_GELU, RES_F32, QKV, GELU_BWD, POS_F32, EPI_F32 = 0, 1, 2, 3, 4, 5, 6
ROWS = 1 << 15          # rows per comparison chunk


@pytest.fixture(scope="module")
def lib(hiplib):
    assert torch.cuda.is_available()
    return hiplib


def need_or_skip(nbytes):
    free = torch.cuda.mem_get_info()[0]
    if free < nbytes:
        pytest.skip(f"needs {nbytes / 2**30:.1f} GiB, {free / 2**30:.1f} GiB free")


class Report:
    def __init__(self, what):
        self.what = what
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        self.t0 = time.perf_counter()

    def done(self):
        torch.cuda.synchronize()
        print(f"\n[large-extents] {self.what}: peak {torch.cuda.max_memory_allocated() / 2**30:.2f} GiB, "
              f"{time.perf_counter() - self.t0:.2f} s")


def stamp_a(rows, lda, tdt):
    """[rows, lda]: the twelve 2-bit fields of the row index, then a one."""
    A = torch.zeros(rows, lda, device=DEV, dtype=tdt)
    m = torch.arange(rows, device=DEV, dtype=torch.int64)
    for i in range(12):
        A[:, i] = ((m >> (2 * i)) & 3).to(tdt)
    A[:, 12] = 1
    return A


def col_codes(dtype, N):
    """(scale s_j, base c_j) as int64 [N]."""
    j = torch.arange(N, device=DEV, dtype=torch.int64)
    if dtype == BF16:
        s = torch.ones_like(j) << (j >> 5)
        return s, s * (128 + 4 * (j & 31))
    return torch.ones_like(j), 4 * j


def stamp_b(dtype, N, K):
    s, c = col_codes(dtype, N)
    B = torch.zeros(N, K, device=DEV, dtype=tdt_of(dtype))
    j = torch.arange(N, device=DEV)
    B[j, j % 12] = s.to(B.dtype)
    B[:, 12] = c.to(B.dtype)
    assert torch.equal(B[:, 12].double(), c.double())        # the codes are exact in the operand type
    return B


def acc_expected(dtype, r0, r1, N):
    """int64 [r1 - r0, N]: the accumulator of rows r0..r1 from coordinates alone."""
    s, c = col_codes(dtype, N)
    m = torch.arange(r0, r1, device=DEV, dtype=torch.int64)[:, None]
    sel = (torch.arange(N, device=DEV, dtype=torch.int64) % 12)[None, :]
    return ((m >> (2 * sel)) & 3) * s[None, :] + c[None, :]


def res_stamp(r0, r1, N):
    m = torch.arange(r0, r1, device=DEV, dtype=torch.int64)[:, None]
    j = torch.arange(N, device=DEV, dtype=torch.int64)[None, :]
    return (m * 3 + j * 7) % 1021


def sign_stamp(r0, r1, N):
    """+16 / -16 by a hash of (row, column): gelu'(+16) = 1 and gelu'(-16) = 0 to well within the GELU bound."""
    m = torch.arange(r0, r1, device=DEV, dtype=torch.int64)[:, None]
    j = torch.arange(N, device=DEV, dtype=torch.int64)[None, :]
    return ((((m * 2654435761) >> 13) + j * 5) & 1) * 32 - 16


def operand_a(dtype):
    """The A operand of a dtype: M_NT + 1 rows, so that `one row more` is in the same allocation.  The caller frees it."""
    need_or_skip((M_NT + 1) * LDA * 2)
    return stamp_a(M_NT + 1, LDA, tdt_of(dtype))


def pow2(e):
    """2^e as float64, exact, for an int64 tensor e (torch.ldexp on the device goes through pow and is not exact)."""
    return ((e + 1023) << 52).view(torch.float64)


NT_CASES = [("nt256", 512, 64, STORE), ("nt256", 512, 64, BIAS_GELU), ("nt256", 512, 64, RES_F32),
            ("nt256", 512, 64, GELU_BWD), ("nt256", 512, 64, POS_F32), ("nt256", 512, 64, EPI_F32),
            ("nt384", 384, 64, STORE), ("nt384", 384, 2048, RES_F32), ("small", 64, 64, STORE),
            ("small_ldo8712", 64, 64, STORE)]


@pytest.mark.parametrize("kernel,N,K,epi", NT_CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("dtype", [BF16, F16], ids=lambda d: kr.DT_NAME[d])
def test_gemm_nt_row_stamps(lib, dtype, kernel, N, K, epi):
    """Every output element of an M = 493 447 launch, exact.  The 256x256 tile takes N = 512, the 384x192 tile N = 384
    (EPI_STORE at any K, EPI_RES_F32 from K = 2048: the dispatch rule of gemm_nt_mfma), the small kernel N = 64.
    With ldo = 8704 the last 16-bit row starts 4608 elements short of element 2^32; `small_ldo8712` repeats the small
    kernel's store with ldo = 8712, where the last 452 rows lie past element 2^32 as well as past byte 2^32.
    EPI_BIAS_GELU: u exact, the activation within the GELU bound of kernel_ref (u |act| + tiny + 4 x the formula's
    deviation).  EPI_GELU_BWD: the pre-activation operand is +-16 by a hash of (row, column), its leading dimension 8704, so
    a misaddressed read flips factors between 1 and 0; bound as in test_kernel_edges_gpu (u |ref| + tiny + |acc| t).
    sgl_op_gemm_nt has no `accumulate` argument, so EPI_F32 is its plain form."""
    M = M_NT
    tdt = tdt_of(dtype)
    f32_out = epi in (RES_F32, POS_F32, EPI_F32)
    odt = torch.float32 if f32_out else tdt
    ldo = 4352 if f32_out else 8712 if kernel == "small_ldo8712" else 8704
    out_bytes = (M + 32) * ldo * (4 if f32_out else 2)
    need_or_skip(3 * out_bytes + (M + 1) * LDA * 2)
    A = operand_a(dtype)
    rep = Report(f"NT {kr.DT_NAME[dtype]} {kernel} N={N} K={K} epi={epi}")
    assert M * LDA * 2 < 2 ** 32 <= (M + 1) * LDA * 2 and M * ldo * (4 if f32_out else 2) > 2 ** 32
    B = stamp_b(dtype, N, K)
    jn = torch.arange(N, device=DEV, dtype=torch.int64)
    bias = (jn % 13).float() if f32_out else torch.zeros(N, device=DEV)
    out = Guarded(M, N, ldo, odt)
    out2 = res = aux = pos = None
    kw = {}
    if epi == BIAS_GELU:
        out2 = Guarded(M, N, ldo, odt)
        kw = dict(out2=out2.ptr, ldo2=ldo)
    if epi == RES_F32:
        res = torch.empty(M, ldo, device=DEV)
        for r0 in range(0, M, ROWS):
            r1 = min(M, r0 + ROWS)
            res[r0:r1, :N] = res_stamp(r0, r1, N).float()
        kw = dict(res=res, ldr=ldo)
    if epi == GELU_BWD:
        aux = torch.empty(M, ldo, device=DEV, dtype=odt)
        for r0 in range(0, M, ROWS):
            r1 = min(M, r0 + ROWS)
            aux[r0:r1, :N] = sign_stamp(r0, r1, N).to(odt)
        kw = dict(aux=aux, ldaux=ldo)
    if epi == POS_F32:
        pos = ((torch.arange(729, device=DEV)[:, None] * 5 + jn[None, :]) % 251).float().contiguous()
        kw = dict(pos=pos, pos_rows=729)
    ok(gemm_nt(lib, dtype, A, LDA, B, K, M, N, K, epi, out.ptr, ldo, bias=None if epi in (STORE, GELU_BWD) else bias, **kw))
    torch.cuda.synchronize()
    what = f"NT stamps {kr.DT_NAME[dtype]} {kernel} epi={epi}"
    out.check(what)
    if out2 is not None:
        out2.check(what + " out2")
    u, tiny = kr.UNIT[odt], kr.TINY[odt]
    for r0 in range(0, M, ROWS):
        r1 = min(M, r0 + ROWS)
        exp = acc_expected(dtype, r0, r1, N)
        got = out.got()[r0:r1]
        if epi == RES_F32:
            exp = exp + res_stamp(r0, r1, N) + (jn % 13)[None, :]
        if epi == POS_F32:
            rows = torch.arange(r0, r1, device=DEV, dtype=torch.int64)[:, None]
            exp = exp + (jn % 13)[None, :] + ((rows % 729) * 5 + jn[None, :]) % 251
        if epi == EPI_F32:
            exp = exp + (jn % 13)[None, :]
        if epi == GELU_BWD:
            uu = sign_stamp(r0, r1, N).double()
            gp = kr.gelu_grad64(uu)
            t = kr.gelu_eval_term(torch.tensor([16.0, -16.0]), grad=True)
            full = exp.double() * gp
            kr.assert_within(got, full, u * full.abs() + tiny + exp.double().abs() * t, f"{what} rows {r0}..{r1}")
            continue
        assert int(exp.max()) < 2 ** 24
        same = got.double() == exp.double()
        if not bool(same.all()):
            bad = (~same).nonzero()[0]
            r, c = int(bad[0]), int(bad[1])
            raise AssertionError(f"{what}: {int((~same).sum())} wrong elements in rows {r0}..{r1}; first at ({r0 + r}, {c}): "
                                 f"got {got[r, c].item()} expected {exp[r, c].item()}")
        if epi == BIAS_GELU:
            act = kr.gelu64(exp.double())
            t = kr.gelu_eval_term(exp[::64].double())
            kr.assert_within(out2.got()[r0:r1], act, u * act.abs() + tiny + t, f"{what} gelu rows {r0}..{r1}")
    rep.done()
    del A, out, out2, res, aux, pos, B
    torch.cuda.empty_cache()


@pytest.mark.parametrize("dtype", [BF16, F16], ids=lambda d: kr.DT_NAME[d])
def test_gemm_nt_one_row_more_is_refused(lib, dtype):
    """M = 493 448 rows of lda = 4352 are 2^32 bytes and 512 more: the launcher refuses (SGL_ERR_UNSUPPORTED from the
    single-kernel entry point; inside the encoder the same refusal would be SGL_ERR_HIP) and the output is untouched."""
    A = operand_a(dtype)
    M, N, K = M_NT + 1, 64, 64
    B = stamp_b(dtype, N, K)
    out = Guarded(M, N, N, tdt_of(dtype))
    assert gemm_nt(lib, dtype, A, LDA, B, K, M, N, K, STORE, out.ptr, N) == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    out.check("refused NT", written=False)
    assert bool(torch.isnan(out.got().float()).all()), "a refused launch wrote its output"
    del A, out, B
    torch.cuda.empty_cache()


@pytest.mark.parametrize("epi", [STORE, RES_F32], ids=lambda e: f"epi{e}")
def test_gemm_f32_generic_row_stamps(lib, epi):
    """The strict fp32 kernel (long indexing, no operand guard) on 493 448 rows of lda = 4352: the operand passes 2^31
    elements and 2^33 bytes; the output and the residual (ldo = ldr = 8712) pass 2^32 elements and 2^34 bytes."""
    M, N, K, ldo = M_NT + 1, 64, 64, 8712
    need_or_skip(M * LDA * 4 + 3 * (M + 32) * ldo * 4)
    rep = Report(f"NT f32 generic epi={epi}")
    assert M * LDA > 2 ** 31 and M * ldo > 2 ** 32
    A = stamp_a(M, LDA, torch.float32)
    B = stamp_b(F16, N, K).float()
    jn = torch.arange(N, device=DEV, dtype=torch.int64)
    bias = (jn % 13).float()
    out = Guarded(M, N, ldo, torch.float32)
    kw, res = {}, None
    if epi == RES_F32:
        res = torch.empty(M, ldo, device=DEV)
        for r0 in range(0, M, ROWS):
            r1 = min(M, r0 + ROWS)
            res[r0:r1, :N] = res_stamp(r0, r1, N).float()
        kw = dict(res=res, ldr=ldo)
    ok(gemm_nt(lib, F32, A, LDA, B, K, M, N, K, epi, out.ptr, ldo, bias=bias, **kw))
    torch.cuda.synchronize()
    out.check("f32 generic stamps")
    for r0 in range(0, M, ROWS):
        r1 = min(M, r0 + ROWS)
        exp = acc_expected(F16, r0, r1, N) + (jn % 13)[None, :]
        if epi == RES_F32:
            exp = exp + res_stamp(r0, r1, N)
        assert torch.equal(out.got()[r0:r1].double(), exp.double()), f"f32 generic epi {epi}: rows {r0}..{r1}"
    rep.done()
    del A, B, out, res
    torch.cuda.empty_cache()


# =========================================================================================================
# QKV scatter at the edge of the row split
# =========================================================================================================
M_QKV = (1 << 22) - 1
QKV_KERNELS = [("nt256", 4, 24, 32), ("nt288", 4, 72, 80), ("small", 1, 8, 8)]


@pytest.mark.parametrize("tokens", [3, 729, 4093, M_QKV], ids=lambda t: f"tokens{t}")
@pytest.mark.parametrize("kernel,heads,hd,hdp", QKV_KERNELS, ids=lambda v: str(v))
def test_qkv_scatter_at_row_split_edge(lib, kernel, heads, hd, hdp, tokens):
    """EPI_QKV on M = 2^22 - 1 rows, the last row count for which qkv_split_row (reciprocal estimate plus one correction)
    is documented exact: every output position against (b * tokens + n) recomputed from its [which][b][h][n][d]
    coordinate, pad columns zero, the rows of the partial last image (where tokens does not divide M) untouched.
    fp16 operands and outputs.  The stamp here: A[m, i] = bit i of m (i < 22), A[m, 22] = 1; row j of B holds a one at
    column j % 22 and 2 j at column 22, so out[m, j] = bit(m, j % 22) + 2 j <= 1727, exact in fp16; any 22 consecutive
    columns name the row, and every head is at least 8 columns of each of q, k, v."""
    dtype = F16
    tdt = tdt_of(dtype)
    M, K = M_QKV, 64
    Nc = 3 * heads * hd
    batch = -(-M // tokens)
    out_rows = 3 * batch * heads * tokens
    need_or_skip(M * K * 2 + 3 * (out_rows + 32) * hdp * 2 + ROWS * Nc * 24)
    rep = Report(f"QKV {kernel} tokens={tokens}")
    # 22 one-bit fields name the row; column code: out[m, j] = bit(m, j % 22) + 2 j  (<= 1 + 2 * 863 = 1727 < 2048)
    A = torch.zeros(M, K, device=DEV, dtype=tdt)
    m = torch.arange(M, device=DEV, dtype=torch.int64)
    for i in range(22):
        A[:, i] = ((m >> i) & 1).to(tdt)
    A[:, 22] = 1
    del m
    jn = torch.arange(Nc, device=DEV, dtype=torch.int64)
    B = torch.zeros(Nc, K, device=DEV, dtype=tdt)
    B[jn, jn % 22] = 1
    B[:, 22] = (2 * jn).to(tdt)
    bias = torch.zeros(Nc, device=DEV)
    out = Guarded(out_rows, hdp, hdp, tdt)
    ok(gemm_nt(lib, dtype, A, K, B, K, M, Nc, K, QKV, out.ptr, 0, bias=bias, tokens=tokens, heads=heads, hd=hd, hdp=hdp,
               batch=batch))
    torch.cuda.synchronize()
    out.check(f"QKV {kernel} tokens={tokens}", written=False)
    got = out.got().view(3, batch, heads, tokens, hdp)
    bstep = max(1, ROWS // tokens)
    d = torch.arange(hdp, device=DEV, dtype=torch.int64)
    bad = torch.zeros((), device=DEV, dtype=torch.int64)
    for which in range(3):
        for h in range(heads):
            col = (which * heads + h) * hd + d                                  # [hdp]; d >= hd is pad
            for b0 in range(0, batch, bstep):
                b1 = min(batch, b0 + bstep)
                for n0 in range(0, tokens, ROWS):
                    n1 = min(tokens, n0 + ROWS)
                    row = (torch.arange(b0, b1, device=DEV, dtype=torch.int64)[:, None] * tokens +
                           torch.arange(n0, n1, device=DEV, dtype=torch.int64)[None, :])[:, :, None]   # [b, n, 1]
                    exp = (((row >> (col % 22)[None, None, :]) & 1) + 2 * col[None, None, :]).double()
                    exp = torch.where(d[None, None, :] < hd, exp, torch.zeros_like(exp))
                    g = got[which, b0:b1, h, n0:n1].double()
                    good = torch.where((row < M).expand_as(exp), g == exp, torch.isnan(g))   # rows past M: untouched
                    bad += (~good).sum()
            assert int(bad) == 0, f"QKV {kernel} tokens={tokens}: {int(bad)} wrong elements up to which={which} head={h}"
    rep.done()
    del A, B, out, got
    torch.cuda.empty_cache()


@pytest.mark.parametrize("dtype", [BF16, F16, F32], ids=lambda d: kr.DT_NAME[d])
def test_qkv_scatter_refuses_2_22_rows(lib, dtype):
    """sgl_op_gemm_nt(EPI_QKV) with M = 2^22 is refused (SGL_ERR_UNSUPPORTED) and writes nothing: the row split is exact below
    2^22 only (include/siglip_hip.h)."""
    M, K, heads, hd, hdp, tokens = 1 << 22, 8, 1, 8, 8, 4
    tdt = tdt_of(dtype)
    A = torch.zeros(M, K, device=DEV, dtype=tdt)
    B = torch.zeros(3 * hd, K, device=DEV, dtype=tdt)
    bias = torch.zeros(3 * hd, device=DEV)
    batch = M // tokens
    out = Guarded(3 * batch * heads * tokens, hdp, hdp, tdt)
    st = gemm_nt(lib, dtype, A, K, B, K, M, 3 * hd, K, QKV, out.ptr, 0, bias=bias, tokens=tokens, heads=heads, hd=hd, hdp=hdp,
                 batch=batch)
    assert st == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    out.check("refused QKV", written=False)
    assert bool(torch.isnan(out.got().float()).all()), "a refused launch wrote its output"
    del A, B, out
    torch.cuda.empty_cache()


# =========================================================================================================
# TN GEMM (dW)
# =========================================================================================================
@pytest.mark.parametrize("case", [("tn6_slabs", 512, 512, 1, 64 << 20), ("tn6_atomic", 512, 512, 1, None),
                                  ("tn_kernel_split1", 256, 256, 1, None), ("tn_kernel_split3_atomic", 256, 256, 3, None),
                                  ("tn_kernel_split3_slabs", 256, 256, 3, 3 * 256 * 256 * 4)], ids=lambda c: c[0])
@pytest.mark.parametrize("dtype", [BF16, F16], ids=lambda d: kr.DT_NAME[d])
def test_gemm_tn_exact_at_operand_guard(lib, dtype, case):
    """dW over Mred = 493 447 rows with lda = ldb = 4352 (both operands 0.1 % under the guard, every split's row base past
    2^31 bytes for the later ones).  A = ones, B[m, j] = ((3 m + 5 j) % 7) - 3: every partial sum is an integer below 2^24 in
    magnitude, so fp32 accumulation is exact in any order (slabs or atomics) and the result equals the int64 column sums."""
    tn_exact(lib, dtype, *case)


def tn_exact(lib, dtype, name, N1, N2, splits, ws_bytes):
    Mred = M_NT
    tdt = tdt_of(dtype)
    need_or_skip(2 * Mred * LDA * 2 + (64 << 20))
    rep = Report(f"TN {kr.DT_NAME[dtype]} {name}")
    A = torch.ones(Mred, LDA, device=DEV, dtype=tdt)
    Bm = torch.zeros(Mred, LDA, device=DEV, dtype=tdt)
    sums = torch.zeros(N2, device=DEV, dtype=torch.int64)
    j = torch.arange(N2, device=DEV, dtype=torch.int64)[None, :]
    for r0 in range(0, Mred, ROWS):
        r1 = min(Mred, r0 + ROWS)
        m = torch.arange(r0, r1, device=DEV, dtype=torch.int64)[:, None]
        v = (3 * m + 5 * j) % 7 - 3
        Bm[r0:r1, :N2] = v.to(tdt)
        sums += v.sum(0)
    assert int(sums.abs().max()) < 2 ** 24
    out = run_gemm_tn(lib, dtype, A, Bm, Mred, N1, N2, N2 + 8, splits=splits, ws_bytes=ws_bytes)
    out.check(f"TN {name}")
    assert torch.equal(out.got().double(), sums.double()[None, :].expand(N1, N2)), f"TN {name}: not the exact column sums"
    rep.done()
    del A, Bm, out
    torch.cuda.empty_cache()


@pytest.mark.parametrize("tile", [256, 384])
def test_gemm_tn_exact_on_each_tile_plan(lib, tile):
    """The 512 x 512 case of test_gemm_tn_exact_at_operand_guard (slabs, bf16) with the tile geometry forced: SGL_TN_TILE is
    read once per process, so a child process runs it, as tests/test_gemm_tn_384_gpu.py does."""
    need_or_skip(2 * M_NT * LDA * 2 + (64 << 20))
    here = os.path.dirname(os.path.abspath(__file__))
    code = (f"import sys; sys.path.insert(0, {here!r}); import __graft_entry__ as e; hl = e.load_package().lib.load(); "
            f"import test_large_extents_gpu as t; t.tn_exact(hl, t.BF16, 'forced_tile', 512, 512, 1, 64 << 20); "
            f"print('TN_EXACT_OK')")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, cwd=os.path.dirname(here),
                       env=dict(os.environ, SGL_TN_TILE=str(tile)))
    assert r.returncode == 0 and "TN_EXACT_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# =========================================================================================================
# Attention maps and the attention forward
# =========================================================================================================
def _lse(q, k, dh, step=4):
    out = torch.empty(q.shape[:3], device=DEV)
    for b in range(0, q.shape[0], step):
        S = (q[b:b + step, ..., :dh].float() @ k[b:b + step, ..., :dh].float().transpose(-1, -2)) * dh ** -0.5
        out[b:b + step] = torch.logsumexp(S, -1)
    return out


@pytest.mark.parametrize("dtype,name", [(BF16, "bf16"), (2, "f32_mfma"), (F32, "f32")], ids=lambda v: str(v))
def test_attn_probs_past_2_31_elements(lib, dtype, name):
    """sgl_op_attn_probs FULL at B = 253, H = 16, N = 729, head 72 / 80: 2 151 273 168 fp32 outputs, 8.6 GB.  Each 4-image
    slice equals, bit for bit, the op called on that slice with offset pointers; four (image, head) slabs (first, the one
    holding byte 2^32, the one holding element 2^31, last) are within the float64 bound of attn_probs_ref; HEAD_MEAN equals
    the FULL output summed over heads in ascending order and divided by H, its defined order."""
    Bn, H, N, dh, DP = 253, 16, 729, 72, 80
    tdt = torch.bfloat16 if dtype == BF16 else torch.float32
    es = 2 if dtype == BF16 else 4
    total = Bn * H * N * N
    assert total > 2 ** 31
    need_or_skip(total * 4 + 2 * Bn * H * N * DP * es + 3 * 4 * H * N * N * 4 + Bn * N * N * 8)
    rep = Report(f"attn_probs {name} B={Bn}")
    g = torch.Generator(device=DEV).manual_seed(7)
    q = torch.zeros(Bn, H, N, DP, device=DEV, dtype=tdt)
    k = torch.zeros(Bn, H, N, DP, device=DEV, dtype=tdt)
    q[..., :dh] = torch.randn(Bn, H, N, dh, device=DEV, generator=g).to(tdt)
    k[..., :dh] = torch.randn(Bn, H, N, dh, device=DEV, generator=g).to(tdt)
    lse = _lse(q, k, dh)
    full = torch.full((Bn, H, N, N), float("nan"), device=DEV)
    ok(lib.sgl_op_attn_probs(dtype, P(q), P(k), P(lse), P(full), Bn, H, N, dh, DP, apr.FULL, stream()))
    torch.cuda.synchronize()
    part = torch.empty(4, H, N, N, device=DEV)
    for b in range(0, Bn, 4):
        nb = min(4, Bn - b)
        part.fill_(float("nan"))
        ok(lib.sgl_op_attn_probs(dtype, P(q[b:]), P(k[b:]), P(lse[b:]), P(part), nb, H, N, dh, DP, apr.FULL, stream()))
        assert torch.equal(full[b:b + nb], part[:nb]), f"attn_probs {name}: images {b}..{b + nb - 1} differ from the sliced call"
    slab = N * N
    for z in (0, 2 ** 32 // (slab * 4), 2 ** 31 // slab, Bn * H - 1):
        b, h = divmod(z, H)
        p, bound = apr.probs_ref(q[b:b + 1, h:h + 1, :, :dh], k[b:b + 1, h:h + 1, :, :dh], lse[b:b + 1, h:h + 1], dtype)
        r = apr.worst_ratio(full[b:b + 1, h:h + 1], p, bound)
        assert r <= 1.0, f"attn_probs {name}: slab (image {b}, head {h}) is {r:.3g} x its float64 bound"
    mean = torch.full((Bn, N, N), float("nan"), device=DEV)
    ok(lib.sgl_op_attn_probs(dtype, P(q), P(k), P(lse), P(mean), Bn, H, N, dh, DP, apr.HEAD_MEAN, stream()))
    torch.cuda.synchronize()
    acc = full[:, 0].clone()
    for h in range(1, H):
        acc += full[:, h]
    acc /= H
    assert torch.equal(mean, acc), f"attn_probs {name}: HEAD_MEAN is not the ascending head sum of FULL over H"
    rep.done()
    del q, k, lse, full, part, mean, acc
    torch.cuda.empty_cache()


def test_attn_fwd_v_base_past_2_32_bytes(lib):
    """sgl_op_attn_fwd, bf16, head-major operands (ld_qkv = 0), B = 1360, H = 16, N = 729: each of q, k, v is 2.54e9 bytes in
    one [3][B][H][N][80] tensor, so the K base lies above 2^31 bytes and the V base above 2^32.  O and LSE of every 8-image
    slice equal the launch on that slice."""
    Bn, H, N, dh, DP = 1360, 16, 729, 72, 80
    D = H * dh
    one = Bn * H * N * DP * 2
    assert one > 2 ** 31 and 2 * one > 2 ** 32
    need_or_skip(3 * one + 2 * Bn * N * D * 2 + Bn * H * N * 4)
    rep = Report(f"attn_fwd bf16 B={Bn}")
    g = torch.Generator(device=DEV).manual_seed(9)
    qkv = torch.zeros(3, Bn, H, N, DP, device=DEV, dtype=torch.bfloat16)
    for j in range(3):
        for b in range(0, Bn, 136):
            qkv[j, b:b + 136, ..., :dh] = torch.randn(136, H, N, dh, device=DEV, generator=g).to(torch.bfloat16)
    out = Guarded(Bn * N, D, D, torch.bfloat16)
    lse = Guarded(1, Bn * H * N, Bn * H * N, torch.float32)
    ok(lib.sgl_op_attn_fwd(BF16, P(qkv[0]), P(qkv[1]), P(qkv[2]), out.ptr, lse.ptr, Bn, H, N, dh, DP, 0, stream()))
    torch.cuda.synchronize()
    out.check("attn_fwd out")
    lse.check("attn_fwd lse")
    O, L = out.got().view(Bn, N, D), lse.got().view(Bn, H, N)
    o8 = torch.empty(8, N, D, device=DEV, dtype=torch.bfloat16)
    l8 = torch.empty(8, H, N, device=DEV)
    for b in range(0, Bn, 8):
        o8.fill_(float("nan"))
        l8.fill_(float("nan"))
        ok(lib.sgl_op_attn_fwd(BF16, P(qkv[0, b:]), P(qkv[1, b:]), P(qkv[2, b:]), P(o8), P(l8), 8, H, N, dh, DP, 0, stream()))
        assert torch.equal(O[b:b + 8], o8) and torch.equal(L[b:b + 8], l8), f"attn_fwd: images {b}..{b + 7}"
    rep.done()
    del qkv, out, lse, O, L, o8, l8
    torch.cuda.empty_cache()


@pytest.mark.parametrize("kind", [0, 1, 2], ids=["dp", "pdp", "relevance"])
@pytest.mark.parametrize("dtype,name", [(BF16, "bf16"), (2, "f32_mfma"), (F32, "f32")], ids=lambda v: str(v))
def test_attn_grad_probs_past_2_31_elements(lib, dtype, name, kind):
    """sgl_op_attn_grad_probs, per-head output (FULL), at the shape of test_attn_probs_past_2_31_elements: each 4-image slice
    of the 2 151 273 168 outputs equals, bit for bit, the op called on that slice with offset pointers, and four
    (image, head) slabs (first, the one holding byte 2^32, the one holding element 2^31, last) are within the float64 bound
    of attn_grad_ref."""
    Bn, H, N, dh, DP = 253, 16, 729, 72, 80
    tdt = torch.bfloat16 if dtype == BF16 else torch.float32
    es = 2 if dtype == BF16 else 4
    need_or_skip(Bn * H * N * N * 4 + 3 * Bn * H * N * DP * es + Bn * N * H * dh * es + 3 * 4 * H * N * N * 4)
    rep = Report(f"attn_grad_probs {name} kind={kind} B={Bn}")
    g = torch.Generator(device=DEV).manual_seed(11 + kind)
    qkv = torch.zeros(3, Bn, H, N, DP, device=DEV, dtype=tdt)
    for j in range(3):
        qkv[j, ..., :dh] = torch.randn(Bn, H, N, dh, device=DEV, generator=g).to(tdt)
    dout = torch.randn(Bn * N, H * dh, device=DEV, generator=g).to(tdt)
    lse = _lse(qkv[0], qkv[1], dh)
    full = torch.full((Bn, H, N, N), float("nan"), device=DEV)
    ok(lib.sgl_op_attn_grad_probs(dtype, P(qkv[0]), P(qkv[1]), P(qkv[2]), P(dout), P(lse), P(full), Bn, H, N, dh, DP, kind,
                                  apr.FULL, stream()))
    torch.cuda.synchronize()
    assert not bool(torch.isnan(full).any()), "output not fully written"
    part = torch.empty(4, H, N, N, device=DEV)
    for b in range(0, Bn, 4):
        nb = min(4, Bn - b)
        part.fill_(float("nan"))
        ok(lib.sgl_op_attn_grad_probs(dtype, P(qkv[0, b:]), P(qkv[1, b:]), P(qkv[2, b:]), P(dout[b * N:]), P(lse[b:]), P(part),
                                      nb, H, N, dh, DP, kind, apr.FULL, stream()))
        assert torch.equal(full[b:b + nb], part[:nb]), f"attn_grad_probs {name}: images {b}..{b + nb - 1} differ"
    slab = N * N
    for z in (0, 2 ** 32 // (slab * 4), 2 ** 31 // slab, Bn * H - 1):
        b, h = divmod(z, H)
        sl = lambda t: t[b:b + 1, h:h + 1, :, :dh]
        do = dout[b * N:(b + 1) * N, h * dh:(h + 1) * dh][None, None]
        x, bound = agr.grad_probs_ref(sl(qkv[0]), sl(qkv[1]), sl(qkv[2]), do, lse[b:b + 1, h:h + 1], dtype, kind)
        r = agr.worst_ratio(full[b:b + 1, h:h + 1], x, bound)
        assert r <= 1.0, f"attn_grad_probs {name} kind {kind}: slab (image {b}, head {h}) is {r:.3g} x its float64 bound"
    rep.done()
    del qkv, dout, lse, full, part
    torch.cuda.empty_cache()


# =========================================================================================================
# MX-fp8 NT GEMM
# =========================================================================================================
def _e4m3(v):
    """The e4m3 byte of a small non-negative integer with at most four significant bits (exact), as uint8."""
    v = v.to(torch.float32)
    e = torch.floor(torch.log2(v.clamp_min(1)))
    mant = (v / torch.exp2(e) - 1) * 8
    assert bool((mant == mant.round()).all())
    byte = ((e + 7) * 8 + mant).to(torch.uint8)
    return torch.where(v == 0, torch.zeros_like(byte), byte)


def test_gemm_nt_mx_row_stamps(lib):
    """gemm_nt_mx, EPI_RES_F32, on M = 991 440 rows (the MX whole-model case) with ldo = ldr = 1152: output and residual are
    4.57e9 bytes each.  Operands are quantised by hand, exactly: integer payloads that e4m3 holds, power-of-two block scales.
    A[m, i] = bits 2i, 2i + 1 of m (i < 12) and a one at columns 32, 64, 96 (all scales 2^0); row j of B holds a one at
    column j % 12 and the octal digits of j at columns 32, 64, 96 as 4 d0 (scale 2^0), d1 (scale 2^5), d2 (scale 2^8), so
    acc[m, j] = field(m, j % 12) + 4 j.  With integer residual and bias stamps every output is an exact integer."""
    M, N, Kp, ld = 991_440, 512, 128, 1152
    need_or_skip(3 * M * ld * 4 + M * Kp * 2)
    rep = Report("MX NT RES_F32 stamps")
    assert M * ld * 4 > 2 ** 32
    m = torch.arange(M, device=DEV, dtype=torch.int64)
    Aq = torch.zeros(M, Kp, device=DEV, dtype=torch.uint8)
    for i in range(12):
        Aq[:, i] = _e4m3((m >> (2 * i)) & 3)
    one = int(_e4m3(torch.ones(1, device=DEV))[0])
    for c in (32, 64, 96):
        Aq[:, c] = one
    As = torch.full((M, Kp // 32), 127, device=DEV, dtype=torch.uint8)
    del m
    j = torch.arange(N, device=DEV, dtype=torch.int64)
    Bq = torch.zeros(N, Kp, device=DEV, dtype=torch.uint8)
    Bq[j, j % 12] = one
    Bq[:, 32] = _e4m3(4 * (j & 7))
    Bq[:, 64] = _e4m3((j >> 3) & 7)
    Bq[:, 96] = _e4m3((j >> 6) & 7)
    Bs = torch.tensor([127, 127, 127 + 5, 127 + 8], device=DEV, dtype=torch.uint8).repeat(N, 1).contiguous()
    bias = (j % 13).float()
    res = torch.empty(M, ld, device=DEV)
    for r0 in range(0, M, ROWS):
        r1 = min(M, r0 + ROWS)
        res[r0:r1, :N] = res_stamp(r0, r1, N).float()
    out = Guarded(M, N, ld, torch.float32)
    ok(lib.sgl_op_gemm_nt_mx(P(Aq), P(As), P(Bq), P(Bs), M, N, Kp, RES_F32, out.ptr, ld, None, P(bias), P(res), ld, 1, 1, 8, 8,
                             1, stream()))
    torch.cuda.synchronize()
    out.check("MX NT stamps")
    for r0 in range(0, M, ROWS):
        r1 = min(M, r0 + ROWS)
        exp = acc_expected(F16, r0, r1, N) + res_stamp(r0, r1, N) + (j % 13)[None, :]
        assert torch.equal(out.got()[r0:r1].double(), exp.double()), f"MX NT stamps: rows {r0}..{r1}"
    rep.done()
    del Aq, As, Bq, Bs, res, out
    torch.cuda.empty_cache()


def _mx_a_fields(M, Kp, nfields, ones_at):
    """MX operand A, all block scales 2^0: A[m, i] = bits 2i, 2i + 1 of m (i < nfields), a one at each column of `ones_at`."""
    m = torch.arange(M, device=DEV, dtype=torch.int64)
    Aq = torch.zeros(M, Kp, device=DEV, dtype=torch.uint8)
    for i in range(nfields):
        Aq[:, i] = _e4m3((m >> (2 * i)) & 3)
    one = int(_e4m3(torch.ones(1, device=DEV))[0])
    for c in ones_at:
        Aq[:, c] = one
    return Aq, torch.full((M, Kp // 32), 127, device=DEV, dtype=torch.uint8), one


def test_gemm_nt_mx_qkv_row_stamps(lib):
    """gemm_nt_mx, EPI_QKV, M = 991 440 = 1360 images of 729 tokens, 16 heads of 72 stored 80 wide: the bf16 output
    [3][1360][16][729][80] is 7.6e9 bytes.  The bf16 stamp of the NT test, s_j (128 + 4 (j & 31) + field(m, j % 10)) with
    s_j = 2^(j >> 5), built from exact MX operands: row j of B holds a one at column j % 10 (block scale s_j), j & 7 at column
    32 (scale 4 s_j), (j >> 3) & 3 at column 64 (scale 32 s_j) and a one at column 96 (scale 128 s_j); A holds the ten 2-bit
    fields of m (m < 2^20) and ones at 32, 64, 96.  Every output position is recomputed from its [which][b][h][n][d]
    coordinate as row b * 729 + n, column which * 1152 + h * 72 + d; pad columns are zero."""
    batch, tokens, heads, hd, hdp, Kp = 1360, 729, 16, 72, 80, 128
    M, Nc = batch * tokens, 3 * heads * hd
    out_rows = 3 * batch * heads * tokens
    need_or_skip(2 * (out_rows + 32) * hdp * 2 + M * Kp * 2 + (1 << 30))
    rep = Report("MX NT QKV stamps")
    assert out_rows * hdp * 2 > 2 ** 32 and M < 2 ** 20
    Aq, As, one = _mx_a_fields(M, Kp, 10, (32, 64, 96))
    j = torch.arange(Nc, device=DEV, dtype=torch.int64)
    e = j >> 5
    Bq = torch.zeros(Nc, Kp, device=DEV, dtype=torch.uint8)
    Bq[j, j % 10] = one
    Bq[:, 32] = _e4m3(j & 7)
    Bq[:, 64] = _e4m3((j >> 3) & 3)
    Bq[:, 96] = one
    Bs = torch.stack((127 + e, 127 + e + 2, 127 + e + 5, 127 + e + 7), 1).to(torch.uint8).contiguous()
    assert int(Bs.max()) < 255
    bias = torch.zeros(Nc, device=DEV)
    out = Guarded(out_rows, hdp, hdp, torch.bfloat16)
    ok(lib.sgl_op_gemm_nt_mx(P(Aq), P(As), P(Bq), P(Bs), M, Nc, Kp, QKV, out.ptr, 0, None, P(bias), None, 0, tokens, heads, hd,
                             hdp, batch, stream()))
    torch.cuda.synchronize()
    out.check("MX QKV stamps")
    got = out.got().view(3, batch, heads, tokens, hdp)
    d = torch.arange(hdp, device=DEV, dtype=torch.int64)
    bstep = ROWS // tokens
    bad = torch.zeros((), device=DEV, dtype=torch.int64)
    zero = torch.zeros((), device=DEV, dtype=torch.float64)
    for which in range(3):
        for h in range(heads):
            col = ((which * heads + h) * hd + d).clamp_max(Nc - 1)             # d >= hd is pad
            scale = pow2(col >> 5)
            for b0 in range(0, batch, bstep):
                b1 = min(batch, b0 + bstep)
                row = (torch.arange(b0, b1, device=DEV, dtype=torch.int64)[:, None] * tokens +
                       torch.arange(tokens, device=DEV, dtype=torch.int64)[None, :])[:, :, None]
                mant = 128 + 4 * (col & 31)[None, None, :] + ((row >> (2 * (col % 10))[None, None, :]) & 3)
                exp = torch.where(d[None, None, :] < hd, mant.double() * scale[None, None, :], zero)
                bad += (got[which, b0:b1, h].double() != exp).sum()
        assert int(bad) == 0, f"MX QKV stamps: {int(bad)} wrong elements up to which={which}"
    rep.done()
    del Aq, As, Bq, Bs, out, got
    torch.cuda.empty_cache()


def test_gemm_nt_mx_bias_gelu_row_stamps(lib):
    """gemm_nt_mx, EPI_BIAS_GELU, M = 991 440, N = ldo = 4352: the fp8 output is 4.31e9 bytes (past 2^32), its scales
    [M][136].  acc[m, j] = 2^(blk % 100) (16 + 2 field(m, j % 10)) with blk = j >> 5: 16, 18, 20 or 22 times a power of two,
    four significant bits, so the MX output represents it exactly whatever block exponent the epilogue picks, and
    gelu(x) = x in fp32 from x = 16 on (the formula's exp2 underflows to 0); bias 0.  The dequantised output (payload times
    2^(scale - 127)) must equal that value exactly: the scale byte places the 32-block, the payload the row.  An fp8
    payload has no room for a column number inside a block: columns j and j + 10 of one block hold the same field."""
    M, N, Kp = 991_440, 4352, 128
    need_or_skip(2 * M * N + M * Kp * 2 + ROWS * N * 40)
    rep = Report("MX NT BIAS_GELU stamps")
    assert M * N > 2 ** 32
    Aq, As, one = _mx_a_fields(M, Kp, 10, (32,))
    j = torch.arange(N, device=DEV, dtype=torch.int64)
    eb = (j >> 5) % 100
    Bq = torch.zeros(N, Kp, device=DEV, dtype=torch.uint8)
    Bq[j, j % 10] = one
    Bq[:, 32] = one
    full = torch.full_like(eb, 127)
    Bs = torch.stack((127 + eb + 1, 127 + eb + 4, full, full), 1).to(torch.uint8).contiguous()
    bias = torch.zeros(N, device=DEV)
    out = torch.full((M + 32, N), 0xAB, device=DEV, dtype=torch.uint8)
    osc = torch.full((M + 32, N // 32), 0xAB, device=DEV, dtype=torch.uint8)
    body, sbody = out[16:16 + M], osc[16:16 + M]
    ok(lib.sgl_op_gemm_nt_mx(P(Aq), P(As), P(Bq), P(Bs), M, N, Kp, BIAS_GELU, body.data_ptr(), N, sbody.data_ptr(), P(bias), None,
                             0, 1, 1, 8, 8, 1, stream()))
    torch.cuda.synchronize()
    for g in (out[:16], out[16 + M:], osc[:16], osc[16 + M:]):
        assert bool((g == 0xAB).all()), "MX BIAS_GELU stamps: guard rows were written"
    bad = torch.zeros((), device=DEV, dtype=torch.int64)
    for r0 in range(0, M, ROWS):
        r1 = min(M, r0 + ROWS)
        m = torch.arange(r0, r1, device=DEV, dtype=torch.int64)[:, None]
        exp = (16 + 2 * ((m >> (2 * (j % 10))[None, :]) & 3)).double() * pow2(eb)[None, :]
        val = body[r0:r1].view(torch.float8_e4m3fn).double()
        val = val * pow2(sbody[r0:r1].to(torch.int64) - 127).repeat_interleave(32, 1)
        bad += (val != exp).sum()
    assert int(bad) == 0, f"MX BIAS_GELU stamps: {int(bad)} wrong elements"
    rep.done()
    del Aq, As, Bq, Bs, out, osc, body, sbody
    torch.cuda.empty_cache()
