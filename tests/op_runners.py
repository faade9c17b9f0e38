"""The LayerNorm, NT GEMM and TN GEMM runners of the GPU kernel tests: one launch through the C ABI on operands the caller made,
every output inside guard bands (`attn_util.Guarded`), nothing compared.  tests/test_kernel_edges_gpu.py checks the
results against float64 bounds, tests/test_nonfinite_gpu.py against the non-finite contract; the attention runner is
`attn_util.launch_attention`."""
import torch

from attn_util import DEV, Guarded, P, ok, stream, tdt_of


def padded(t, ld, fill=float("nan")):
    """[rows, w] -> the same values as the first w columns of a [rows, ld] matrix whose slack holds `fill`."""
    out = torch.full((t.shape[0], ld), fill, device=t.device, dtype=t.dtype)
    out[:, :t.shape[1]] = t
    return out


def gemm_nt(lib, dtype, A, lda, B, ldb, M, N, K, epi, out, ldo, out2=None, ldo2=0, bias=None, res=None, ldr=0, aux=None,
            ldaux=0, pos=None, pos_rows=1, tokens=1, heads=1, hd=8, hdp=8, batch=1):
    return lib.sgl_op_gemm_nt(dtype, P(A), lda, P(B), ldb, M, N, K, epi, out, ldo, out2, ldo2, P(bias), P(res), ldr,
                              P(aux), ldaux, P(pos), pos_rows, tokens, heads, hd, hdp, batch, stream())


def run_gemm_nt(lib, dtype, M, N, K, epi, A, B, bias=None, res=None, aux=None, pos=None):
    """One NT GEMM launch of epilogue 0, 1, 2, 4, 5 or 6.  A [M, lda >= K], B [N, ldb >= K] in the operand dtype, bias [N]
    fp32 (NULL when None), res [M, ldr >= N] fp32 (epilogue 2), aux [M, ldaux >= N] in the output dtype (4), pos [rows, N]
    fp32 (5); the leading dimensions are the operands' own row strides.  The outputs get ldo = N + 8 (out) and N + 16
    (out2, epilogue 1) with guard bands; returns (out, out2 or None), accepted, synchronised, unchecked."""
    tdt = tdt_of(dtype)
    odt = torch.float32 if epi in (2, 5, 6) else tdt
    ldo = N + 8
    out = Guarded(M, N, ldo, odt)
    out2 = None
    kw = {}
    if epi == 1:
        out2 = Guarded(M, N, N + 16, odt)
        kw = dict(out2=out2.ptr, ldo2=N + 16)
    if epi == 2:
        kw = dict(res=res, ldr=res.stride(0))
    if epi == 4:
        kw = dict(aux=aux, ldaux=aux.stride(0))
    if epi == 5:
        kw = dict(pos=pos, pos_rows=pos.shape[0])
    ok(gemm_nt(lib, dtype, A, A.stride(0), B, B.stride(0), M, N, K, epi, out.ptr, ldo, bias=bias, **kw))
    torch.cuda.synchronize()
    return out, out2


def run_gemm_nt_qkv(lib, dtype, A, B, bias, batch, tokens, heads, hd, hdp):
    """The QKV scatter epilogue (3): A [batch * tokens, lda], B [3 * heads * hd, ldb] in the operand dtype, bias fp32.
    Returns the `Guarded` [3 * batch * heads * tokens, hdp] output (the [3][B][H][N][hdp] tensor), unchecked."""
    D = heads * hd
    out = Guarded(3 * batch * heads * tokens, hdp, hdp, tdt_of(dtype))
    ok(gemm_nt(lib, dtype, A, A.stride(0), B, B.stride(0), batch * tokens, 3 * D, D, 3, out.ptr, 0, bias=bias,
               tokens=tokens, heads=heads, hd=hd, hdp=hdp, batch=batch))
    torch.cuda.synchronize()
    return out


def run_layernorm(lib, x, gam, bet, dy, dr, odt_code, dy_code, lp_code, dgamma=True, dbeta=True, eps=1e-6):
    """sgl_op_layernorm_fwd then _bwd from the forward's own statistics, as the encoder does.  x [M, D], gam, bet fp32; dy
    in dtype `dy_code`; dr fp32 or None.  Returns the `Guarded` outputs y, mean, rstd, dx, dx_lp, dgamma, dbeta (the last
    two None when not asked for), accepted, synchronised, unchecked."""
    M, D = x.shape
    y = Guarded(M, D, D, tdt_of(odt_code))
    mean = Guarded(1, M, M, torch.float32)
    rstd = Guarded(1, M, M, torch.float32)
    ok(lib.sgl_op_layernorm_fwd(P(x), P(gam), P(bet), y.ptr, odt_code, mean.ptr, rstd.ptr, M, D, eps, stream()))
    dx = Guarded(M, D, D, torch.float32)
    dxlp = Guarded(M, D, D, tdt_of(lp_code))
    dg = Guarded(1, D, D, torch.float32) if dgamma else None
    db = Guarded(1, D, D, torch.float32) if dbeta else None
    nblk = max(1, min(768, (M + 3) // 4))
    scratch = torch.empty(nblk * 3 * D, device=DEV)
    ok(lib.sgl_op_layernorm_bwd(P(dy), dy_code, P(x), mean.ptr, rstd.ptr, P(gam), P(dr), dx.ptr, dxlp.ptr, lp_code,
                                dg.ptr if dg else None, db.ptr if db else None, P(scratch), scratch.numel() * 4, M, D,
                                stream()))
    torch.cuda.synchronize()
    return dict(y=y, mean=mean, rstd=rstd, dx=dx, dx_lp=dxlp, dgamma=dg, dbeta=db)


def run_gemm_tn(lib, dtype, A, B, Mred, N1, N2, ldo, splits=1, accumulate=0, prior=None, ws_bytes=None):
    """sgl_op_gemm_tn (ws_bytes None) or sgl_op_gemm_tn_ws with `ws_bytes` of scratch.  A [>= Mred, lda >= N1],
    B [>= Mred, ldb >= N2] in the operand dtype, the leading dimensions their own row strides; the output [N1, N2] fp32
    with leading dimension ldo starts as `prior` (accumulate) or NaN.  Returns the `Guarded` output, accepted,
    synchronised, unchecked."""
    out = Guarded(N1, N2, ldo, torch.float32, prior=prior)
    if ws_bytes is None:
        ok(lib.sgl_op_gemm_tn(dtype, P(A), A.stride(0), P(B), B.stride(0), Mred, N1, N2, splits, out.ptr, ldo, accumulate,
                              stream()))
    else:
        ws = torch.empty(max(ws_bytes, 16), device=DEV, dtype=torch.uint8)
        ok(lib.sgl_op_gemm_tn_ws(dtype, P(A), A.stride(0), P(B), B.stride(0), Mred, N1, N2, splits, out.ptr, ldo,
                                 accumulate, P(ws), ws_bytes, stream()))
    torch.cuda.synchronize()
    return out


def run_pool_attn_fwd(lib, dtype, q, K, V, B, H, N, dh, DP):
    """sgl_op_pool_attn_fwd: q [H * dh] fp32, K, V head-major [B, H, N, DP] in the operand dtype.  Returns the `Guarded`
    out [B, H * dh] and probs [B * H, N] (fp32), accepted, synchronised, unchecked."""
    tdt = tdt_of(dtype)
    out, probs = Guarded(B, H * dh, H * dh, tdt), Guarded(B * H, N, N, torch.float32)
    ok(lib.sgl_op_pool_attn_fwd(dtype, P(q), P(K), P(V), out.ptr, probs.ptr, B, H, N, dh, DP, stream()))
    torch.cuda.synchronize()
    return out, probs


def run_pool_attn_bwd(lib, dtype, q, K, V, probs, dout, B, H, N, dh, DP):
    """sgl_op_pool_attn_bwd from the fp32 probabilities `probs` [B, H, N] the caller passes (a pointer or a tensor).
    Returns the `Guarded` dkv [B * N, 2 * H * dh] and dq [B, H * dh] (fp32)."""
    tdt = tdt_of(dtype)
    dkv, dq = Guarded(B * N, 2 * H * dh, 2 * H * dh, tdt), Guarded(B, H * dh, H * dh, torch.float32)
    pp = probs if isinstance(probs, int) else P(probs)
    ok(lib.sgl_op_pool_attn_bwd(dtype, P(q), P(K), P(V), pp, P(dout), dkv.ptr, dq.ptr, B, H, N, dh, DP, stream()))
    torch.cuda.synchronize()
    return dkv, dq
