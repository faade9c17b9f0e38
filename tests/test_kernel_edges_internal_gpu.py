"""GPU tests of the HIP kernels only the encoder calls, through the thin ``sgl_op_*`` entry points at the end of
csrc/encoder.hip: the pooling head's one-query attention, the position-table resize backward, the weight-shadow casts,
the bf16x3 operand splits, and the small sums and copies (csrc/attention_pool.hip, csrc/elementwise.hip, csrc/layernorm.hip).

Same discipline as tests/test_kernel_edges_gpu.py and tests/test_kernel_edges_aux_gpu.py: every output element against a
float64 reference of the same operation on the same rounded inputs (tests/kernel_ref.py; tests/test_kernel_ref_host.py
asserts the bounds against CPU emulations), every output between sentinel guard rows (and guard columns where the kernel
takes a leading dimension), the body NaN or, where the kernel accumulates, a non-zero prior.  No element is excused.
Casts, copies and splits are held to bit equality.  Each case is named after the branch it is there for; the shapes are
the smallest that reach it.
"""
import ctypes as C

import pytest
import torch

import kernel_ref as kr
from kernel_ref import BF16, EPS32, F16, F32
from op_runners import run_pool_attn_bwd, run_pool_attn_fwd
from test_kernel_edges_aux_gpu import untouched, within
from test_kernel_edges_gpu import DEV, Guarded, P, gen, lib, ok, randn, rup, stream, tdt_of  # noqa: F401  (lib: fixture)

pytestmark = pytest.mark.gpu
OK, BAD_SHAPE, UNSUPPORTED, WORKSPACE, NULL = 0, -1, -2, -3, -5
TYPES = [F32, BF16, F16]
TYPE_IDS = [kr.DT_NAME[d] for d in TYPES]


class Flat(Guarded):
    """A guarded 1-D output of any length: one guard row either side and guard elements up to the next multiple of 8
    (which also keeps the body 16-byte aligned)."""
    G = 1

    def __init__(self, n, tdt, prior=None):
        super().__init__(1, n, rup(n, 8), tdt, prior)


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bits(got, ref, what, nonfinite_by_class=False):
    """Bit equality (so -0 != +0 and every NaN payload counts).  nonfinite_by_class: where the reference is NaN or +-inf
    the class has to agree (NaN with NaN, +-inf with the same inf) and the bits are free: the sign and payload of a NaN
    that an operation makes (inf - inf) differ between devices."""
    assert got.shape == ref.shape and got.dtype == ref.dtype, f"{what}: {got.shape} {got.dtype} vs {ref.shape} {ref.dtype}"
    ref = ref.to(got.device)
    ne = bits(got) != bits(ref)
    if nonfinite_by_class:
        g, r = got.float(), ref.float()
        special = ~torch.isfinite(r)
        ne = torch.where(special, ~((torch.isnan(g) & torch.isnan(r)) | (g == r)), ne)
    assert not bool(ne.any()), f"{what}: {int(ne.sum())} of {ne.numel()} elements differ in bits, first at " \
                               f"{ne.flatten().nonzero()[0].item()}"


def misaligned(t):
    """The same values in a buffer that starts 4 bytes off 16-byte alignment."""
    buf = torch.empty(t.numel() + 8, device=t.device, dtype=t.dtype)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


# =========================================================================================================
# sgl_op_pool_attn_fwd / _bwd
# =========================================================================================================
# (head_dim, head_dim_pad): CPR = DP / 8 chunk columns, RP = 256 / CPR rows per pass, 256 - RP * CPR idle threads
POOL_DIMS = [("dp16_cpr2", 8, 16), ("dp64_cpr8_divides256", 64, 64), ("dp80_cpr10_rp25_6idle", 72, 80),
             ("dp96_cpr12_4idle", 88, 96)]
POOL_FWD_MAX, POOL_BWD_MAX = 1488, 1364                  # DP 80: floor(16376 / 11), floor(16376 / 12)


def pool_case(lib, dtype, kind, B, H, N, dh, DP, what, fwd=True, bwd=True):
    """One forward and one backward launch, every output guarded and bounded.  The backward gets the float64
    probabilities rounded to fp32, so its check does not inherit the forward's error."""
    tdt = tdt_of(dtype)
    q, K, V, do = kr.pool_inputs(kind, B, H, N, dh, DP, tdt, seed=B + H)
    assert bool((K[..., dh:] == 0).all()) and bool((V[..., dh:] == 0).all())            # the layout contract
    qd, Kd, Vd, dod = q.to(DEV), K.to(DEV), V.to(DEV), do.to(DEV)
    (rP, bP), (ro, bo) = kr.pool_attn_fwd_ref(q, K, V, H, dh, tdt)
    if fwd:
        out, probs = run_pool_attn_fwd(lib, dtype, qd, Kd, Vd, B, H, N, dh, DP)
        out.check(what + " out")
        probs.check(what + " probs")
        got_p = probs.got().reshape(B, H, N).cpu()
        within(got_p, rP, bP, f"pool_attn_fwd {what} probs")
        rows = (got_p.double().sum(-1) - 1).abs()
        assert bool((rows <= bP.sum(-1) + N * EPS32).all()), f"{what}: probabilities do not sum to 1 ({rows.max():.3g})"
        within(out.got(), ro, bo, f"pool_attn_fwd {what} out")
    if bwd:
        p32 = rP.float()
        pd = p32.to(DEV)
        dkv, dq = run_pool_attn_bwd(lib, dtype, qd, Kd, Vd, pd, dod, B, H, N, dh, DP)
        dkv.check(what + " dkv")                        # written=True: every element of [B*N][2*H*dh]
        dq.check(what + " dq_partial")
        (rkv, bkv), (rq, bq) = kr.pool_attn_bwd_ref(q, K, V, p32, do, H, dh, tdt)
        within(dkv.got(), rkv, bkv, f"pool_attn_bwd {what} dkv")
        within(dq.got(), rq, bq, f"pool_attn_bwd {what} dq_partial")


@pytest.mark.parametrize("kind", ["gauss", "big_scores_one_dominant", "equal_scores"])
@pytest.mark.parametrize("dims", POOL_DIMS, ids=lambda d: d[0])
@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
def test_pool_attn_rows_per_pass_and_softmax_stride(lib, dtype, dims, kind):
    """N = 1, RP - 1, RP, RP + 1 (the chunk-partial loop's first, last and second trip for the case's RP) and 255, 256,
    257 (the 256-stride softmax loops), for (B, H) = (1, 1) and (2, 3) with a different query per head."""
    name, dh, DP = dims
    RP = 256 // (DP // 8)
    for B, H in ((1, 1), (2, 3)):
        for N in sorted({1, RP - 1, RP, RP + 1, 255, 256, 257}):
            pool_case(lib, dtype, kind.split("_")[0], B, H, N, dh, DP, f"{name} {kr.DT_NAME[dtype]} {kind} B{B}H{H} N={N}")


@pytest.mark.parametrize("N", [100, 300, POOL_BWD_MAX, POOL_FWD_MAX],
                         ids=["N100_below_lds_floor", "N300_above_lds_floor", "N1364_bwd_max", "N1488_fwd_max"])
@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
def test_pool_attn_lds_floor_and_largest_accepted_n(lib, dtype, N):
    """DP 80: N * CPR below and above the 2048-float floor of the shared LDS region, and the largest N each launcher
    accepts (1364 backward, 1488 forward), which must pass the same bounds."""
    pool_case(lib, dtype, "gauss", 2, 3, N, 72, 80, f"dp80 {kr.DT_NAME[dtype]} N={N}", bwd=N <= POOL_BWD_MAX)


@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
def test_pool_attn_one_token_more_is_refused_untouched(lib, dtype):
    """N = 1489 forward and N = 1365 backward at DP 80: SGL_ERR_UNSUPPORTED, nothing written; NULL and shape errors too."""
    B, H, dh, DP = 1, 2, 72, 80
    tdt = tdt_of(dtype)
    N = POOL_FWD_MAX + 1
    q, K, V, do = (t.to(DEV) for t in kr.pool_inputs("gauss", B, H, N, dh, DP, tdt, seed=1))
    out, probs = Guarded(B, H * dh, H * dh, tdt), Guarded(B * H, N, N, torch.float32)
    dkv, dq = Guarded(B * N, 2 * H * dh, 2 * H * dh, tdt), Guarded(B, H * dh, H * dh, torch.float32)
    pr = torch.full((B, H, N), 1.0 / N, device=DEV)

    def fwd(N_=N, q_=P(q), out_=out.ptr, dh_=dh, dt=dtype):
        return lib.sgl_op_pool_attn_fwd(dt, q_, P(K), P(V), out_, probs.ptr, B, H, N_, dh_, DP, stream())

    def bwd(N_=POOL_BWD_MAX + 1, p_=P(pr), dkv_=dkv.ptr, dh_=dh, dt=dtype):
        return lib.sgl_op_pool_attn_bwd(dt, P(q), P(K), P(V), p_, P(do), dkv_, dq.ptr, B, H, N_, dh_, DP, stream())
    assert fwd() == UNSUPPORTED and bwd() == UNSUPPORTED and bwd(N_=POOL_FWD_MAX) == UNSUPPORTED
    assert fwd(q_=None) == NULL and fwd(out_=None) == NULL and bwd(p_=None) == NULL and bwd(dkv_=None) == NULL
    assert fwd(N_=0) == BAD_SHAPE and fwd(dh_=70) == BAD_SHAPE and fwd(dh_=88) == BAD_SHAPE and bwd(N_=0) == BAD_SHAPE
    assert fwd(N_=8, dt=2) == UNSUPPORTED and bwd(N_=8, dt=5) == UNSUPPORTED
    assert bwd(N_=8, dkv_=dkv.ptr + 4) == UNSUPPORTED
    torch.cuda.synchronize()
    for b in (out, probs, dkv, dq):
        untouched(b, "pool_attn refusal")


# =========================================================================================================
# sgl_op_pos_resize_bwd
# =========================================================================================================
@pytest.mark.parametrize("D", [4, 5, 144], ids=lambda d: f"D{d}")
@pytest.mark.parametrize("grid", kr.POS_BWD_GRIDS, ids=lambda g: f"{g[0]}to{g[1]}x{g[2]}")
def test_pos_resize_bwd_grids(lib, grid, D):
    """Every grid of test_posresize_rect plus the identity (3, 3, 3), a steep upscale (2, 37, 5: up to 185 outputs per
    table entry, all of them in the scanned range or lost) and a steep downscale (27, 1, 1: most entries get nothing).
    The kernel ADDS: the prior is non-zero and part of the reference.  Then the adjoint identity with sgl_op_pos_resize
    within the two bounds, and bit-identical results from two calls."""
    g0, gh, gw = grid
    g = gen(g0 * 1000 + gh * 10 + gw + D)
    dout, prior, T = randn(g, gh * gw, D), randn(g, g0 * g0, D), randn(g, g0 * g0, D)
    what = f"pos_resize_bwd {g0}->{gh}x{gw} D={D}"
    outs = []
    for _ in range(2):
        dt_ = Guarded(g0 * g0, D, D, torch.float32, prior=prior)
        ok(lib.sgl_op_pos_resize_bwd(P(dout), gh, gw, dt_.ptr, g0, D, stream()))
        dt_.check(what)
        outs.append(dt_.got().clone())
    same_bits(outs[0], outs[1], what + " (two calls)")
    ref, bound = kr.pos_resize_bwd_ref(dout.cpu(), g0, gh, gw, prior.cpu())
    within(outs[0], ref, bound, what)
    # <R T, G> == <T, R^T G>
    zero = Guarded(g0 * g0, D, D, torch.float32, prior=torch.zeros(g0 * g0, D, device=DEV))
    ok(lib.sgl_op_pos_resize_bwd(P(dout), gh, gw, zero.ptr, g0, D, stream()))
    fwd = Guarded(gh * gw, D, D, torch.float32)
    ok(lib.sgl_op_pos_resize(P(T), g0, fwd.ptr, gh, gw, D, stream()))
    fwd.check(what + " forward")
    lhs = (fwd.got().double() * dout.double()).sum().item()
    rhs = (T.double() * zero.got().double()).sum().item()
    _, b0 = kr.pos_resize_bwd_ref(dout.cpu(), g0, gh, gw, torch.zeros(g0 * g0, D))
    tol = (kr.pos_resize_bound(T.cpu(), g0)[None, :] * dout.cpu().double().abs()).sum().item() + \
        (T.cpu().double().abs() * b0).sum().item()
    print(f"RATIO pos_resize_adjoint {abs(lhs - rhs) / tol:.4f}  {what}")
    assert abs(lhs - rhs) <= tol, f"{what}: adjoint identity off by {abs(lhs - rhs):.3g} (allowed {tol:.3g})"


def test_pos_resize_bwd_refusals_write_nothing(lib):
    dout = torch.ones(6, 4, device=DEV)
    dt_ = Guarded(9, 4, 4, torch.float32)
    assert lib.sgl_op_pos_resize_bwd(None, 2, 3, dt_.ptr, 3, 4, stream()) == NULL
    assert lib.sgl_op_pos_resize_bwd(P(dout), 2, 3, None, 3, 4, stream()) == NULL
    for gh, gw, g0, D in ((0, 3, 3, 4), (2, 0, 3, 4), (2, 3, 0, 4), (2, 3, 3, 0)):
        assert lib.sgl_op_pos_resize_bwd(P(dout), gh, gw, dt_.ptr, g0, D, stream()) == BAD_SHAPE
    torch.cuda.synchronize()
    untouched(dt_, "pos_resize_bwd refusal")


# =========================================================================================================
# sgl_op_cast_pad / sgl_op_cast_job
# =========================================================================================================
CAST_R = [1, 63, 64, 65]
CAST_C = [1, 3, 4, 5, 63, 64, 65, 538]


def cast_source(R, C, lds, seed, off):
    """src [R][C] inside an [R][lds] fp32 matrix whose slack is NaN, 16-byte aligned or 4 bytes off."""
    full = torch.full((R, lds), float("nan"), device=DEV)
    body = (randn(gen(seed), R, C) * 3).reshape(-1)
    k = min(body.numel() // 2, 3)                        # NaN and +-inf where there is room: the class has to arrive
    body[body.numel() - k:] = torch.tensor([float("nan"), float("inf"), -float("inf")], device=DEV)[:k]
    full[:, :C] = body.view(R, C)
    return misaligned(full) if off else full


def padded_ref(src, R, C, Rp, Cp, tdt):
    ref = torch.zeros(Rp, Cp, device=DEV, dtype=tdt)
    ref[:R, :C] = src[:, :C].to(tdt)
    return ref


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "src_4_bytes_off"])
@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
def test_cast_pad_every_shape_bit_exact(lib, dtype, off):
    """R in {1, 63, 64, 65} x C in {1, 3, 4, 5, 63, 64, 65, 538} with Rp > R, Cp > C, ldd > Cp and lds % 4 != 0: torch's
    round-to-nearest, exact zeros in the padding, guards intact."""
    tdt = tdt_of(dtype)
    for R in CAST_R:
        for C_ in CAST_C:
            Rp, Cp, lds = R + 5, C_ + 3, C_ + 1 + (C_ % 4 == 3)
            ldd = Cp + 5
            src = cast_source(R, C_, lds, R * 1000 + C_, off)
            dst = Guarded(Rp, Cp, ldd, tdt)
            ok(lib.sgl_op_cast_pad(P(src), R, C_, lds, dst.ptr, dtype, Rp, Cp, ldd, stream()))
            what = f"cast_pad {kr.DT_NAME[dtype]} {R}x{C_}"
            dst.check(what, written=False)            # the source holds NaN: same_bits proves the writes
            same_bits(dst.got(), padded_ref(src, R, C_, Rp, Cp, tdt), what, nonfinite_by_class=True)


class Job:
    """sgl_cast_mat / sgl_cast_vec tables plus the guarded destinations and their references."""

    def __init__(self, pkg, tdt):
        self.L, self.tdt = pkg.lib, tdt
        self.mats, self.vecs, self.checks, self.keep = [], [], [], []

    def mat(self, R, C_, lds, Rp, Cp, ldd, ldt, off=0, want_dst=True, want_t=True, seed=0):
        src = cast_source(R, C_, lds, seed + R * 1000 + C_, off)
        ref = padded_ref(src, R, C_, Rp, Cp, self.tdt)
        dst = Guarded(Rp, Cp, ldd, self.tdt) if want_dst else None
        dst_t = Guarded(Cp, Rp, ldt, self.tdt) if want_t else None
        self.mats.append(self.L.SglCastMat(P(src), dst.ptr if dst else None, dst_t.ptr if dst_t else None, R, C_, lds, Rp,
                                           Cp, ldd, ldt))
        self.keep.append(src)
        tag = f"{R}x{C_}->{Rp}x{Cp}"
        if dst:
            self.checks.append((dst, ref, tag + " dst"))
        if dst_t:
            self.checks.append((dst_t, ref.t().contiguous(), tag + " dst_t"))

    def vec(self, n, np_, seed=0):
        src = randn(gen(seed + n), max(n, 1))
        dst = Flat(np_, torch.float32)
        ref = torch.zeros(1, np_, device=DEV)
        ref[0, :n] = src[:n]
        self.vecs.append(self.L.SglCastVec(P(src), dst.ptr, n, np_))
        self.keep.append(src)
        self.checks.append((dst, ref, f"vec {n}->{np_}"))

    def run(self, lib, dtype):
        m = (self.L.SglCastMat * max(len(self.mats), 1))(*self.mats)
        v = (self.L.SglCastVec * max(len(self.vecs), 1))(*self.vecs)
        return lib.sgl_op_cast_job(m if self.mats else None, len(self.mats), v if self.vecs else None, len(self.vecs),
                                   dtype, stream())

    def verify(self, what):
        for buf, ref, tag in self.checks:
            buf.check(f"{what} {tag}", written=False)    # (the sources hold NaN: same_bits proves the writes)
            same_bits(buf.got(), ref, f"{what} {tag}", nonfinite_by_class=True)


# name -> (source 4 bytes off, lds(C), Rp(R), Cp(C), ldd(Cp), ldt(Rp), dst, dst_t)
CAST_JOB_VARIANTS = {
    "vector_load_vector_stores": (0, lambda c: rup(c, 4), lambda r: rup(r + 1, 16), lambda c: rup(c + 1, 8),
                                  lambda cp: cp + 8, lambda rp: rp + 8, True, True),
    "scalar_load_src_misaligned": (1, lambda c: rup(c, 4), lambda r: rup(r + 1, 16), lambda c: rup(c + 1, 8),
                                   lambda cp: cp + 8, lambda rp: rp + 8, True, True),
    "scalar_load_lds_mod4": (0, lambda c: rup(c, 4) + 1, lambda r: rup(r + 1, 16), lambda c: rup(c + 1, 8),
                             lambda cp: cp + 8, lambda rp: rp + 8, True, True),
    "scalar_store_ldd_odd": (0, lambda c: rup(c, 4), lambda r: rup(r + 1, 16), lambda c: c + 3,
                             lambda cp: cp + 1 + cp % 2, lambda rp: rp + 8, True, True),
    "partial_transposed_store_rp_mod16_ldt_odd": (0, lambda c: rup(c, 4), lambda r: r + 5, lambda c: rup(c + 1, 8),
                                                  lambda cp: cp + 8, lambda rp: rp + 1 + rp % 2, True, True),
    "dst_t_null": (0, lambda c: rup(c, 4), lambda r: r + 5, lambda c: c + 3, lambda cp: cp + 5, lambda rp: rp, True, False),
    "dst_null": (0, lambda c: rup(c, 4), lambda r: r + 5, lambda c: c + 3, lambda cp: cp, lambda rp: rp + 3, False, True),
}


@pytest.mark.parametrize("variant", CAST_JOB_VARIANTS, ids=str)
@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
def test_cast_job_load_and_store_paths(pkg, lib, dtype, variant):
    """One-matrix jobs over R in {1, 63, 64, 65} x C in {1, 3, 4, 5, 63, 64, 65, 538}: the 16-byte and the scalar load,
    the vector and the scalar row store, the 16-element and the partial transposed store, either destination absent.
    Both destinations guarded (rows and the columns up to ldd / ldt) and bit-exact, zeros in the padding."""
    off, lds, Rp, Cp, ldd, ldt, want_dst, want_t = CAST_JOB_VARIANTS[variant]
    for R in CAST_R:
        for C_ in CAST_C:
            job = Job(pkg, tdt_of(dtype))
            rp, cp = Rp(R), Cp(C_)
            job.mat(R, C_, lds(C_), rp, cp, ldd(cp), ldt(rp), off, want_dst, want_t)
            ok(job.run(lib, dtype))
            job.verify(f"cast_job {variant} {kr.DT_NAME[dtype]}")


@pytest.mark.parametrize("shape", ["six_matrices_four_vectors", "vectors_only", "matrices_only", "hostile_fc1_538_rows"])
@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
def test_cast_job_tables(pkg, lib, dtype, shape):
    """Six differently shaped matrices (the tile0 search: 1, 2, 4, 27, 9 and 1 tiles) plus four vectors with np > n in one
    launch; a job of vectors only; of matrices only; the hostile fc1 weight (538 rows padded to 640)."""
    job = Job(pkg, tdt_of(dtype))
    if shape in ("six_matrices_four_vectors", "matrices_only"):
        for i, (R, C_, Rp, Cp) in enumerate([(5, 7, 16, 8), (65, 33, 80, 40), (100, 70, 112, 72), (144, 538, 144, 544),
                                             (538, 1, 544, 8), (64, 64, 64, 64)]):
            job.mat(R, C_, C_ + i, Rp, Cp, Cp + 8 * (i % 2), Rp + 8 * (i % 3), off=i % 2, want_t=i != 2, seed=i)
    if shape in ("six_matrices_four_vectors", "vectors_only"):
        for n, np_ in ((1, 8), (144, 256), (538, 640), (257, 300)):
            job.vec(n, np_)
    if shape == "hostile_fc1_538_rows":
        job.mat(538, 144, 144, 640, 144, 144, 640)
        job.vec(538, 640)
    ok(job.run(lib, dtype))
    job.verify(f"cast_job {shape} {kr.DT_NAME[dtype]}")


def test_cast_job_refusals_write_nothing(pkg, lib):
    """Seven matrices or five vectors: SGL_ERR_BAD_SHAPE; a NULL source, Rp < R, ldd < Cp: refused, nothing written."""
    L = pkg.lib
    job = Job(pkg, torch.bfloat16)
    job.mat(5, 7, 8, 16, 8, 8, 16)
    job.vec(3, 8)
    m7, v5 = (L.SglCastMat * 7)(*([job.mats[0]] * 7)), (L.SglCastVec * 5)(*([job.vecs[0]] * 5))
    assert lib.sgl_op_cast_job(m7, 7, None, 0, BF16, stream()) == BAD_SHAPE
    assert lib.sgl_op_cast_job(None, 0, v5, 5, BF16, stream()) == BAD_SHAPE
    assert lib.sgl_op_cast_job(None, 1, None, 0, BF16, stream()) == NULL
    assert lib.sgl_op_cast_job(None, 7, None, 0, BF16, stream()) == NULL           # NULL is looked at before the counts
    both = L.SglCastMat.from_buffer_copy(job.mats[0])
    both.src, both.Rp = None, 4
    assert lib.sgl_op_cast_job((L.SglCastMat * 1)(both), 1, None, 0, BF16, stream()) == NULL
    good = job.mats[0]
    for field, val, want in (("src", None, NULL), ("Rp", 4, BAD_SHAPE), ("ldd", 7, BAD_SHAPE), ("ldt", 15, BAD_SHAPE),
                             ("lds", 6, BAD_SHAPE)):
        bad = L.SglCastMat.from_buffer_copy(good)
        setattr(bad, field, val)
        assert lib.sgl_op_cast_job((L.SglCastMat * 1)(bad), 1, None, 0, BF16, stream()) == want, field
    assert lib.sgl_op_cast_job((L.SglCastMat * 1)(good), 1, None, 0, 2, stream()) == UNSUPPORTED
    src = torch.ones(5, 8, device=DEV)
    dst = Guarded(16, 8, 8, torch.bfloat16)
    assert lib.sgl_op_cast_pad(P(src), 5, 7, 8, dst.ptr, BF16, 4, 8, 8, stream()) == BAD_SHAPE
    assert lib.sgl_op_cast_pad(None, 5, 7, 8, dst.ptr, BF16, 16, 8, 8, stream()) == NULL
    assert lib.sgl_op_cast_pad(P(src), 5, 7, 8, dst.ptr, 5, 16, 8, 8, stream()) == UNSUPPORTED
    torch.cuda.synchronize()
    untouched(dst, "cast_pad refusal")
    for buf, _, tag in job.checks:
        untouched(buf, "cast_job refusal " + tag)


# =========================================================================================================
# sgl_op_split3
# =========================================================================================================
def split_source(R, C_, ld, seed, off):
    x = randn(gen(seed), R, C_) * torch.logspace(-8, 8, C_, device=DEV)[None, :]
    sp = kr.split3_special_values().to(DEV)
    flat_ = x.view(-1)
    k = min(flat_.numel(), sp.numel())
    flat_[:k] = sp[:k]
    if flat_.numel() >= 2 * sp.numel():                  # again at the other end: another position within the 8-chunk
        flat_[-sp.numel():] = sp
    full = torch.full((R, ld), float("nan"), device=DEV)
    full[:, :C_] = x
    return misaligned(full) if off else full


@pytest.mark.parametrize("src_kind", ["aligned_ld_mod4_0", "src_4_bytes_off", "ld_mod4_1"])
@pytest.mark.parametrize("C_", [8, 9, 15, 144], ids=lambda c: f"C{c}")
@pytest.mark.parametrize("stacked", [0, 1], ids=["rows", "stack"])
@pytest.mark.parametrize("b_side", [0, 1], ids=["a_side", "b_side"])
def test_split3_segments_bit_exact(lib, b_side, stacked, C_, src_kind):
    """hi = bf16(x), lo = bf16(x - hi) bit for bit in the documented segment / plane order, zeros from C to Cs.  The source
    holds +-0, fp32 subnormals, bf16 rounding ties and the largest values that stay finite in bf16.  C = 8: whole chunks;
    9 and 15: a partial last chunk (the scalar load); 144: the model's.  Vector loads need ld % 4 == 0 and an aligned src."""
    R, Cs = 5, rup(C_, 8)
    ld = rup(C_, 4) + (1 if src_kind == "ld_mod4_1" else 4)
    x = split_source(R, C_, ld, C_ * 10 + b_side, src_kind == "src_4_bytes_off")
    out = Guarded(3 * R, Cs, Cs, torch.bfloat16) if stacked else Guarded(R, 3 * Cs, 3 * Cs, torch.bfloat16)
    ok(lib.sgl_op_split3(P(x), R, C_, ld, out.ptr, Cs, b_side, stacked, stream()))
    what = f"split3 {'stack' if stacked else 'rows'} b_side={b_side} C={C_} {src_kind}"
    out.check(what, written=False)                        # the source holds NaN: same_bits proves the writes
    same_bits(out.got(), kr.split3_layout(x[:, :C_], Cs, b_side, stacked), what, nonfinite_by_class=True)
    hi, lo = kr.split3_ref(x[:, :C_])
    normal = (x[:, :C_].abs() >= 2.0 ** -100) & torch.isfinite(x[:, :C_])
    rec = hi.double() + lo.double()
    assert bool(((rec - x[:, :C_].double()).abs()[normal] <= 2.0 ** -17 * x[:, :C_].double().abs()[normal]).all())


@pytest.mark.parametrize("stacked,b_side", [(0, 1), (1, 0)], ids=["rows_b_side", "stack_a_side"])
def test_split3_grid_stride_second_trip(lib, stacked, b_side):
    """4100 x 4096: 2 099 200 eight-element chunks, more than the 8192 x 256 threads of the capped grid."""
    R, C_ = 4100, 4096
    assert R * (C_ // 8) > 8192 * 256
    x = randn(gen(41), R, C_)
    out = Guarded(3 * R, C_, C_, torch.bfloat16) if stacked else Guarded(R, 3 * C_, 3 * C_, torch.bfloat16)
    ok(lib.sgl_op_split3(P(x), R, C_, C_, out.ptr, C_, b_side, stacked, stream()))
    out.check("split3 grid-stride")
    same_bits(out.got(), kr.split3_layout(x, C_, b_side, stacked), "split3 grid-stride")


def test_split3_refusals_write_nothing(lib):
    x = torch.ones(5, 16, device=DEV)
    out = Guarded(5, 48, 48, torch.bfloat16)
    assert lib.sgl_op_split3(None, 5, 9, 16, out.ptr, 16, 0, 0, stream()) == NULL
    assert lib.sgl_op_split3(P(x), 5, 9, 16, out.ptr, 24, 0, 0, stream()) == BAD_SHAPE      # Cs != round_up(C, 8)
    assert lib.sgl_op_split3(P(x), 5, 9, 8, out.ptr, 16, 0, 0, stream()) == BAD_SHAPE       # ld < C
    assert lib.sgl_op_split3(P(x), 5, 9, 16, out.ptr + 2, 16, 0, 0, stream()) == UNSUPPORTED
    torch.cuda.synchronize()
    untouched(out, "split3 refusal")


# =========================================================================================================
# sums: sgl_op_batch_sum, sgl_op_vecmat, sgl_op_reduce_partials, _partials3, sgl_op_reduce_splits
# =========================================================================================================
def prior_of(accumulate, g, *shape):
    """accumulate: a finite prior that is part of the reference; overwrite: the NaN body, which must vanish."""
    return randn(g, *shape) * 5 if accumulate else None


@pytest.mark.parametrize("accumulate", [0, 1], ids=["overwrite", "accumulate"])
def test_batch_sum_sizes(lib, accumulate):
    """B in {1, 7} x n in {1, 255, 256, 257}: one block short, exact, and one element into the second block."""
    for B in (1, 7):
        for n in (1, 255, 256, 257):
            g = gen(B * 1000 + n)
            x = randn(g, B, n)
            prior = prior_of(accumulate, g, 1, n)
            out = Flat(n, torch.float32, prior)
            ok(lib.sgl_op_batch_sum(P(x), B, n, out.ptr, accumulate, stream()))
            what = f"batch_sum B={B} n={n} acc={accumulate}"
            out.check(what)
            ref, bound = kr.sum_ref(x.cpu(), None if prior is None else prior[0].cpu())
            within(out.got()[0], ref, bound, what)


@pytest.mark.parametrize("accumulate", [0, 1], ids=["overwrite", "accumulate"])
@pytest.mark.parametrize("rows", [1, 15, 16, 17, 144, 1152], ids=lambda r: f"rows{r}")
def test_vecmat_row_chunks(lib, rows, accumulate):
    """rows below, at and above the 16 row chunks (rows = 1, 15, 17: empty chunks, which must still write their zero
    partial) x cols in {1, 63, 64, 65, 144}.  The 16 x cols scratch is an output too: guarded and fully written."""
    for cols in (1, 63, 64, 65, 144):
        g = gen(rows * 1000 + cols)
        v, W = randn(g, rows), randn(g, rows, cols)
        prior = prior_of(accumulate, g, 1, cols)
        out, scratch = Flat(cols, torch.float32, prior), Guarded(16, cols, cols, torch.float32)
        blank = Flat(cols, torch.float32)
        assert lib.sgl_op_vecmat(P(v), P(W), rows, cols, scratch.ptr, 16 * cols * 4 - 1, blank.ptr, accumulate,
                                 stream()) == WORKSPACE
        ok(lib.sgl_op_vecmat(P(v), P(W), rows, cols, scratch.ptr, 16 * cols * 4, out.ptr, accumulate, stream()))
        what = f"vecmat rows={rows} cols={cols} acc={accumulate}"
        out.check(what)
        scratch.check(what + " scratch")
        untouched(blank, what + " (scratch one byte short)")
        ref, bound = kr.vecmat_ref(v.cpu(), W.cpu(), None if prior is None else prior[0].cpu())
        within(out.got()[0], ref, bound, what)


@pytest.mark.parametrize("accumulate", [0, 1], ids=["overwrite", "accumulate"])
@pytest.mark.parametrize("nblk", [1, 7, 8, 9, 16, 17, 24, 25], ids=lambda b: f"nblk{b}")
def test_reduce_partials_row_groups(lib, nblk, accumulate):
    """nblk either side of the 8 row groups and of the two-rows-per-trip loop x n in {1, 31, 32, 33}, stride > n with NaN
    in the slack columns."""
    for n in (1, 31, 32, 33):
        g = gen(nblk * 100 + n)
        stride = n + 3
        part = torch.full((nblk, stride), float("nan"), device=DEV)
        part[:, :n] = randn(g, nblk, n)
        prior = prior_of(accumulate, g, 1, n)
        out = Flat(n, torch.float32, prior)
        ok(lib.sgl_op_reduce_partials(P(part), nblk, stride, out.ptr, n, accumulate, stream()))
        what = f"reduce_partials nblk={nblk} n={n} acc={accumulate}"
        out.check(what)
        ref, bound = kr.sum_ref(part[:, :n].cpu(), None if prior is None else prior[0].cpu())
        within(out.got()[0], ref, bound, what)


@pytest.mark.parametrize("null", [None, 0, 1, 2], ids=["all_outputs", "o0_null", "o1_null", "o2_null"])
@pytest.mark.parametrize("nblk", [1, 24, 25, 33, 57], ids=lambda b: f"nblk{b}")
@pytest.mark.parametrize("n", [5, 32, 33], ids=["n5_one_group_three_outputs", "n32_aligned", "n33_group_spans_two_outputs"])
def test_reduce_partials3_outputs_and_flags(lib, n, nblk, null):
    """n % 32 != 0 puts two (n = 5: all three) outputs into one 32-column workgroup.  Each output NULL in turn (the other
    two still right), all eight combinations of the three accumulate flags, nblk either side of the four-rows-per-trip
    loop (24 + 8 g) and of its remainder loop."""
    stride = 3 * n + 5
    g = gen(n * 100 + nblk)
    part = torch.full((nblk, stride), float("nan"), device=DEV)
    part[:, :3 * n] = randn(g, nblk, 3 * n)
    for flags in range(8):
        acc = [(flags >> k) & 1 for k in range(3)]
        priors = [prior_of(acc[k], g, 1, n) for k in range(3)]
        outs = [Flat(n, torch.float32, priors[k]) for k in range(3)]
        ptrs = [None if k == null else outs[k].ptr for k in range(3)]
        ok(lib.sgl_op_reduce_partials3(P(part), nblk, stride, ptrs[0], ptrs[1], ptrs[2], n, acc[0], acc[1], acc[2], stream()))
        for k in range(3):
            what = f"reduce_partials3 n={n} nblk={nblk} null={null} acc={acc} out{k}"
            if k == null:
                outs[k].check(what, written=False)
                if priors[k] is None:
                    untouched(outs[k], what)
                else:
                    same_bits(outs[k].got(), priors[k], what + " (skipped output changed)")
                continue
            outs[k].check(what)
            ref, bound = kr.sum_ref(part[:, k * n:(k + 1) * n].cpu(), None if priors[k] is None else priors[k][0].cpu())
            within(outs[k].got()[0], ref, bound, what)


SPLIT_CASES = [(sh, sp) for sh in ((3, 8), (65, 132)) for sp in (1, 2, 5)] + [((1152, 2048), 2)]


@pytest.mark.parametrize("accumulate", [0, 1], ids=["overwrite", "accumulate"])
@pytest.mark.parametrize("shape,splits", SPLIT_CASES,
                         ids=[f"{a}x{b}_splits{sp}" + ("_grid_stride" if a > 1000 else "") for (a, b), sp in SPLIT_CASES])
def test_reduce_splits_fixed_order_fold(lib, shape, splits, accumulate):
    """splits in {1, 2, 5} slabs with stride above N1 * N2 into an output with ldo > N2 (guard columns); 1152 x 2048 is
    589 824 float4s, more than the 2048 x 256 threads of the capped grid."""
    N1, N2 = shape
    g = gen(N1 + N2 + splits)
    stride, ldo = N1 * N2 + 8, N2 + 4
    ws = torch.full((splits, stride), float("nan"), device=DEV)
    ws[:, :N1 * N2] = randn(g, splits, N1 * N2)
    prior = prior_of(accumulate, g, N1, N2)
    out = Guarded(N1, N2, ldo, torch.float32, prior)
    ok(lib.sgl_op_reduce_splits(P(ws), splits, stride, N1, N2, out.ptr, ldo, accumulate, stream()))
    what = f"reduce_splits {N1}x{N2} splits={splits} acc={accumulate}"
    out.check(what)
    ref, bound = kr.sum_ref(ws[:, :N1 * N2].reshape(splits, N1, N2), prior)
    within(out.got(), ref, bound, what)


def test_reduce_splits_refusals_write_nothing(lib):
    """N2 % 4, ldo % 4, a misaligned out or ws, stride % 4: SGL_ERR_UNSUPPORTED before any launch."""
    ws = torch.ones(2 * 64 + 8, device=DEV)
    out = Guarded(4, 8, 12, torch.float32)

    def call(ws_=P(ws), stride=36, N2=8, out_=out.ptr, ldo=12, splits=2, N1=4):
        return lib.sgl_op_reduce_splits(ws_, splits, stride, N1, N2, out_, ldo, 0, stream())
    assert call(N2=6) == UNSUPPORTED and call(ldo=14) == UNSUPPORTED and call(stride=38) == UNSUPPORTED
    assert call(out_=out.ptr + 4) == UNSUPPORTED and call(ws_=P(ws) + 4) == UNSUPPORTED
    assert call(ws_=None) == NULL and call(out_=None) == NULL
    assert call(splits=0) == BAD_SHAPE and call(ldo=4) == BAD_SHAPE and call(stride=28) == BAD_SHAPE
    torch.cuda.synchronize()
    untouched(out, "reduce_splits refusal")


# =========================================================================================================
# sgl_op_add_f32 (b NULL: the copy) and sgl_op_cast_f32
# =========================================================================================================
SMALL_N = [1, 3, 4, 5, 1027]
BIG_N = 4096 * 256 * 4 + 7 + 4096          # above the capped grid's one trip of float4s, with a 3-element tail


@pytest.mark.parametrize("with_b", [0, 1], ids=["copy_b_null", "add"])
@pytest.mark.parametrize("n", SMALL_N + [BIG_N], ids=lambda n: f"n{n}")
def test_add_and_copy_f32_tail_and_grid_stride(lib, n, with_b):
    """n < 4 (tail only), n % 4 in {0, 1, 3}, and one n past 4096 x 256 float4s plus a tail.  The copy is bit-exact; the
    sum is the one fp32 addition (bound 2 x 2^-24 (|a| + |b|), and bit-equal to torch's a + b)."""
    g = gen(n % 1000 + with_b)
    a = randn(g, n)
    b = randn(g, n) if with_b else None
    out = Flat(n, torch.float32)
    ok(lib.sgl_op_add_f32(P(a), P(b), out.ptr, n, stream()))
    what = f"{'add' if with_b else 'copy'}_f32 n={n}"
    out.check(what)
    if not with_b:
        same_bits(out.got()[0], a, what)
        return
    ref, bound = kr.sum_ref(torch.stack([a, b]))
    within(out.got()[0], ref, bound, what)
    same_bits(out.got()[0], a + b, what)


@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
def test_cast_f32_sizes(lib, dtype):
    """The three destination types at every small n and past the 4096 x 256 threads of the capped grid: torch's
    round-to-nearest, bit for bit."""
    tdt = tdt_of(dtype)
    for n in SMALL_N + [BIG_N]:
        a = randn(gen(n % 1000), n) * 100
        out = Flat(n, tdt)
        ok(lib.sgl_op_cast_f32(P(a), out.ptr, dtype, n, stream()))
        what = f"cast_f32 {kr.DT_NAME[dtype]} n={n}"
        out.check(what)
        same_bits(out.got()[0], a.to(tdt), what)


def test_add_and_cast_f32_refusals_write_nothing(lib):
    """copy_f32_kernel moves float4s without looking at its pointers: the entry point refuses one 4 bytes off."""
    a = torch.ones(64 + 8, device=DEV)
    out = Flat(64, torch.float32)
    assert lib.sgl_op_add_f32(P(a) + 4, None, out.ptr, 64, stream()) == UNSUPPORTED
    assert lib.sgl_op_add_f32(P(a), P(a) + 4, out.ptr, 64, stream()) == UNSUPPORTED
    assert lib.sgl_op_add_f32(P(a), None, out.ptr + 4, 60, stream()) == UNSUPPORTED
    assert lib.sgl_op_add_f32(None, None, out.ptr, 64, stream()) == NULL
    assert lib.sgl_op_cast_f32(P(a), None, BF16, 64, stream()) == NULL
    assert lib.sgl_op_cast_f32(P(a), out.ptr, 2, 64, stream()) == UNSUPPORTED
    torch.cuda.synchronize()
    untouched(out, "add_f32 / cast_f32 refusal")
