"""CPU: the rules of tests/nonfinite_util.py on hand-made masks, and the conditions of tests/test_nonfinite_gpu.py that
involve the float64 references alone, for every case of its tables: the excused set of a NaN poison is empty (every
element that a finite change of the site moves is non-finite in the NaN run), a +-inf poison makes nothing non-finite
that NaN leaves finite, and at most half of a site's dependent elements are excused.  So a failure of the GPU test is
the kernel's.  The excused share of every case is printed (pytest -s)."""
import pytest
import torch

import kernel_ref as kr
import nonfinite_util as nf
from kernel_ref import BF16, F32

NAN, INF = nf.NAN, nf.INF


# ---------------------------------------------------------------------------------------------------------------
# the rules on hand-made masks
# ---------------------------------------------------------------------------------------------------------------
def _t(*v, dt=torch.float32):
    return torch.tensor(v, dtype=dt)


def _m(*v):
    return torch.tensor(v, dtype=torch.bool)


def test_rules_pass_and_count_excused():
    clean = _t(1.0, 2.0, 3.0, 4.0)
    got = _t(1.0, NAN, INF, 7.0)                  # 0 independent, 1 and 2 must, 3 excused (dependent, finite for this inf)
    exc, dep = nf.apply_rules("op", clean, got, _m(0, 1, 1, 1), _m(0, 1, 1, 0))
    assert (exc, dep) == (1, 3)


def test_rule1_names_the_swallowed_element_with_bits():
    clean, got = _t(1.0, 2.0), _t(1.0, 0.0)
    with pytest.raises(AssertionError, match=r"myop q\[1\]=nan -> O: rule 1 .*first at \(1,\).*0x00000000.*0x40000000"):
        nf.apply_rules("myop q[1]=nan -> O", clean, got, _m(0, 1), _m(0, 1))


def test_rule1_accepts_inf_for_nan():
    nf.apply_rules("op", _t(1.0), _t(-INF), _m(1), _m(1))


def test_rule2_is_bitwise():
    clean = _t(0.0, 1.0)
    with pytest.raises(AssertionError, match=r"rule 2 .*first at \(0,\).*0x80000000.*0x00000000"):
        nf.apply_rules("op", clean, _t(-0.0, 1.0), _m(0, 0), _m(0, 0))       # -0.0 == 0.0, but not in bits
    one_ulp = torch.nextafter(_t(1.0, dt=torch.bfloat16), _t(2.0, dt=torch.bfloat16))
    with pytest.raises(AssertionError, match="rule 2 .*0x3f81.*0x3f80"):
        nf.apply_rules("op", _t(1.0, dt=torch.bfloat16), one_ulp, _m(0), _m(0))
    nf.apply_rules("op", _t(NAN), _t(NAN), _m(0), _m(0))                     # the same NaN bits are the same bits


def test_rule2_catches_a_nan_that_spread():
    with pytest.raises(AssertionError, match="rule 2"):
        nf.apply_rules("op", _t(1.0, 2.0), _t(NAN, NAN), _m(0, 1), _m(0, 1))


def test_rule2_with_a_bound_replaces_bits_only_on_independent_elements():
    clean, ref = _t(1.0, 2.0), _t(1.0, 2.0).double()
    nf.apply_rules("op", clean, _t(1.0 + 1e-6, NAN), _m(0, 1), _m(0, 1), ref, _t(1e-5, 0.0))
    with pytest.raises(AssertionError, match="rule 2 .*float64 bound"):
        nf.apply_rules("op", clean, _t(1.0 + 1e-4, NAN), _m(0, 1), _m(0, 1), ref, _t(1e-5, 0.0))
    with pytest.raises(AssertionError, match="rule 2"):                       # a NaN is outside every bound
        nf.apply_rules("op", clean, _t(NAN, NAN), _m(0, 1), _m(0, 1), ref, _t(1e-5, 0.0))


def test_excused_elements_are_not_asserted():
    nf.apply_rules("op", _t(1.0), _t(5.0), _m(1), _m(0))
    nf.apply_rules("op", _t(1.0), _t(NAN), _m(1), _m(0))


def test_poison_and_perturb_leave_the_clean_inputs_alone():
    inp = dict(a=torch.arange(1.0, 7.0).view(2, 3), b=None)
    p = nf.poison(inp, ("a", 4), NAN)
    assert torch.isnan(p["a"][1, 1]) and bool(torch.isfinite(inp["a"]).all()) and p["b"] is None
    assert nf.site_name(inp, ("a", 4)) == "a[1, 1]"
    assert [n for n, _ in nf.site_values(("a", 4, ("nan", "-inf")))] == ["nan", "-inf"] and \
        nf.site_values(("a", 4)) == nf.VALUES
    m = nf.perturbed(inp, ("a", 4))
    assert m["a"][1, 1].item() not in (inp["a"][1, 1].item(),) and int((m["a"] != inp["a"]).sum()) == 1
    assert bool((nf.nonzero(torch.tensor([0.0, 2.0, -0.0])) == torch.tensor([1.0, 2.0, 1.0])).all())


def test_reference_conditions_catch_a_reference_that_drops_nan():
    inp = dict(x=torch.tensor([1.0, -2.0, 3.0]))
    with pytest.raises(AssertionError, match="excused set of a NaN poison is not empty"):
        nf.reference_conditions("relu", lambda d: dict(y=d["x"].double().clamp_min(0.0).nan_to_num(0.0)), inp, ("x", 0))
    with pytest.raises(AssertionError, match="more than half"):               # exp(-inf) = 0: everything excused
        nf.reference_conditions("exp", lambda d: dict(y=torch.exp(-d["x"].double().abs())), inp, ("x", 0))
    refs, shares = nf.reference_conditions("sum", lambda d: dict(y=d["x"].double().sum(0, keepdim=True)), inp, ("x", 2))
    assert shares == {"nan": 0.0, "+inf": 0.0, "-inf": 0.0} and torch.isnan(refs["nan"]["y"]).all()


def test_drive_end_to_end_on_a_cpu_stand_in():
    """The driver with an fp32 torch row-centering standing in for the kernel: it passes; a stand-in that swallows (the
    row mean is formed from cleaned values) fails rule 1 and one that couples rows through a shared mean fails rule 2,
    each naming op, site, value and output."""
    g = torch.Generator().manual_seed(0)
    inp = dict(x=nf.nonzero(torch.randn(3, 5, generator=g)))
    sites = [("x", 0), ("x", 14, ("nan", "+inf"))]
    ref = lambda d: dict(c=d["x"].double() - d["x"].double().mean(-1, keepdim=True), s=d["x"].double().sum(-1))
    good = lambda d, poisoned: dict(c=d["x"] - d["x"].mean(-1, keepdim=True), s=d["x"].sum(-1))
    st = nf.drive("center", good, ref, inp, sites)
    assert st.cases == 5 and st.worst == 0.0
    swallow = lambda d, poisoned: dict(c=d["x"] - d["x"].nan_to_num(0.0, 0.0, 0.0).mean(-1, keepdim=True), s=d["x"].sum(-1))
    with pytest.raises(AssertionError, match=r"center x\[0, 0\]=nan -> c: rule 1 .*first at \(0, 1\)"):
        nf.drive("center", swallow, ref, inp, sites)
    coupled = lambda d, poisoned: dict(c=d["x"] - d["x"].mean(), s=d["x"].sum(-1))
    with pytest.raises(AssertionError, match=r"center x\[0, 0\]=nan -> c: rule 2 .*first at \(1, 0\)"):
        nf.drive("center", coupled, ref, inp, sites)


# ---------------------------------------------------------------------------------------------------------------
# the case tables: conditions on the references
# ---------------------------------------------------------------------------------------------------------------
def conditions(op, ref, inputs, sites):
    st = nf.Stats(op)
    for site in sites:
        _, shares = nf.reference_conditions(op, ref, inputs, site)
        assert shares["nan"] == 0.0
        for vn, _ in nf.site_values(site):
            st.add(f"{nf.site_name(inputs, site)}={vn}", shares[vn])
    print(st.line())
    return st


@pytest.mark.parametrize("N,dh", nf.ATTN_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("dtype", nf.ATTN_DTYPES, ids=lambda d: kr.DT_NAME[d])
def test_attention_reference_conditions(dtype, N, dh):
    inp = nf.attn_inputs(dtype, N, dh)
    conditions(f"attention {kr.DT_NAME[dtype]} N={N} dh={dh}", nf.attn_ref, inp, nf.attn_sites(inp))


def test_attention_reference_granularity():
    """What the contract asks the kernels to reproduce (B = 2, H = 2, N = 33, dh = 8, NaN at [1, 0, 32, 7]): q -> row 32
    of O, lse and dQ, all of dK and dV; v -> column 7 of O, dV finite, all of dQ and dK; dout -> column 7 of dV (row 32 of dQ,
    all of dK); nothing in the other three heads."""
    N, dh = nf.ATTN_SHAPES[0]
    inp = nf.attn_inputs(F32, N, dh)
    site = lambda o: (o, nf.flat((2, 2, N, dh), (1, 0, N - 1, dh - 1)))
    head = lambda t: nf.nonfinite(t)[1, 0]
    row = torch.zeros(N, dh, dtype=torch.bool)
    row[N - 1] = True
    col = torch.zeros(N, dh, dtype=torch.bool)
    col[:, dh - 1] = True
    full, none = torch.ones(N, dh, dtype=torch.bool), torch.zeros(N, dh, dtype=torch.bool)
    want = dict(q=dict(O=row, dQ=row, dK=full, dV=full), k=dict(O=full, dQ=full, dK=full, dV=full),
                v=dict(O=col, dQ=full, dK=full, dV=none), dout=dict(O=none, dQ=row, dK=full, dV=col))
    for o, masks in want.items():
        r = nf.attn_ref(nf.poison(inp, site(o), NAN))
        for name, m in masks.items():
            assert torch.equal(head(r[name]), m), f"{o} -> {name}"
        for name, t in r.items():
            other = nf.nonfinite(t).clone()
            other[1, 0] = False
            assert not bool(other.any()), f"{o} -> {name}: another head is touched"
    assert torch.equal(head(nf.attn_ref(nf.poison(inp, site("q"), NAN))["lse"]), row[:, 0])


@pytest.mark.parametrize("dres", [True, False], ids=["dres", "no_dres"])
@pytest.mark.parametrize("dtype", nf.LN_DTYPES, ids=lambda d: kr.DT_NAME[d])
@pytest.mark.parametrize("D", nf.LN_D, ids=lambda d: f"D{d}")
def test_layernorm_reference_conditions(D, dtype, dres):
    inp = nf.ln_inputs(D, dtype, dres)
    conditions(f"layernorm {kr.DT_NAME[dtype]} D={D}", nf.ln_ref, inp, nf.ln_sites(D))


def test_layernorm_reference_granularity():
    """x -> that row of y, mean, rstd, dx and all of dgamma (dbeta untouched); dy -> that row of dx, one column each of
    dgamma and dbeta; gamma -> that column of y, all of dx."""
    D = 516
    inp = nf.ln_inputs(D, BF16, True)
    nz = lambda t: nf.nonfinite(t).nonzero().tolist()
    r = nf.ln_ref(nf.poison(inp, ("x", nf.flat((nf.LN_M, D), (4, D - 1))), NAN))
    assert nz(r["mean"]) == [[4]] and nz(r["rstd"]) == [[4]] and not nz(r["dbeta"])
    assert bool(nf.nonfinite(r["dgamma"]).all())
    for n in ("y", "dx"):
        assert torch.equal(nf.nonfinite(r[n]).all(1), torch.tensor([0, 0, 0, 0, 1], dtype=torch.bool))
        assert not bool(nf.nonfinite(r[n])[:4].any())
    r = nf.ln_ref(nf.poison(inp, ("dy", nf.flat((nf.LN_M, D), (0, 0))), NAN))
    assert not nz(r["y"]) and nz(r["dgamma"]) == [[0]] and nz(r["dbeta"]) == [[0]]
    assert bool(nf.nonfinite(r["dx"])[0].all()) and not bool(nf.nonfinite(r["dx"])[1:].any())
    r = nf.ln_ref(nf.poison(inp, ("gamma", D - 1), NAN))
    assert bool(nf.nonfinite(r["y"])[:, D - 1].all()) and not bool(nf.nonfinite(r["y"])[:, :D - 1].any())
    assert bool(nf.nonfinite(r["dx"]).all()) and not nz(r["dgamma"]) and not nz(r["dbeta"])


@pytest.mark.parametrize("epi", nf.NT_EPIS, ids=lambda e: f"epi{e}")
@pytest.mark.parametrize("M", nf.NT_M, ids=lambda m: f"M{m}")
@pytest.mark.parametrize("dtype", nf.NT_DTYPES, ids=lambda d: kr.DT_NAME[d])
def test_gemm_nt_reference_conditions(dtype, M, epi):
    inp = nf.nt_inputs(dtype, M, epi)
    conditions(f"gemm_nt {kr.DT_NAME[dtype]} M={M} epi={epi}", nf.nt_ref(epi), inp, nf.nt_sites(M, epi))


def test_gemm_nt_wide_reference_conditions():
    M, N, K, epi = nf.NT_WIDE
    inp = nf.nt_inputs(BF16, M, epi, N, K)
    conditions(f"gemm_nt bf16 M={M} N={N} K={K} epi={epi}", nf.nt_ref(epi), inp, nf.nt_sites(M, epi, N, K))


@pytest.mark.parametrize("shape", nf.QKV_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("dtype", nf.NT_DTYPES, ids=lambda d: kr.DT_NAME[d])
def test_gemm_nt_qkv_reference_conditions(dtype, shape):
    conditions(f"gemm_nt qkv {kr.DT_NAME[dtype]} {shape}", nf.qkv_ref(*shape), nf.qkv_inputs(dtype, *shape),
               nf.qkv_sites(*shape))


@pytest.mark.parametrize("accumulate", [0, 1], ids=["store", "accumulate"])
@pytest.mark.parametrize("route", nf.TN_ROUTES + nf.TN_FALLBACKS, ids=lambda r: r[0])
@pytest.mark.parametrize("dtype", nf.TN_DTYPES, ids=lambda d: kr.DT_NAME[d])
def test_gemm_tn_reference_conditions(dtype, route, accumulate):
    name, Mred, N2 = route[:3]
    inp = nf.tn_inputs(dtype, Mred, N2, accumulate)
    conditions(f"gemm_tn {kr.DT_NAME[dtype]} {name}", nf.tn_ref, inp, nf.tn_sites(Mred, N2))
    r = nf.tn_ref(nf.poison(inp, ("A", nf.flat((Mred, nf.TN_N), (Mred - 1, 0))), NAN))["out"]
    assert bool(nf.nonfinite(r)[0].all()) and not bool(nf.nonfinite(r)[1:].any())          # row 0 of dW, nothing else
    r = nf.tn_ref(nf.poison(inp, ("B", nf.flat((Mred, N2), (Mred - 1, N2 - 1))), NAN))["out"]
    assert bool(nf.nonfinite(r)[:, N2 - 1].all()) and not bool(nf.nonfinite(r)[:, :N2 - 1].any())


@pytest.mark.parametrize("D", nf.LN_MX_D, ids=lambda d: f"D{d}")
def test_layernorm_mx_reference_conditions(D):
    conditions(f"layernorm_fwd_mx D={D}", nf.ln_mx_ref, nf.ln_mx_inputs(D), nf.ln_mx_sites(D))


def test_mx_gemm_reference_conditions():
    conditions("quantize_mxfp8 + gemm_nt_mx", nf.mx_gemm_ref, nf.mx_gemm_inputs(), nf.mx_gemm_sites())


@pytest.mark.parametrize("dims", nf.POOL_DIMS, ids=lambda d: f"dh{d[0]}")
@pytest.mark.parametrize("dtype", nf.POOL_DTYPES, ids=lambda d: kr.DT_NAME[d])
def test_pool_attention_reference_conditions(dtype, dims):
    dh, DP = dims
    inp = nf.pool_inputs(dtype, dh, DP)
    conditions(f"pool_attn {kr.DT_NAME[dtype]} dh={dh}", nf.pool_ref(dh), inp, nf.pool_sites(inp, dh))
    r = nf.pool_ref(dh)(nf.poison(inp, ("K", nf.flat(tuple(inp["K"].shape), (1, 0, 0, 0))), NAN))
    for name in ("out", "dq"):                                                  # image 0 is untouched
        assert not bool(nf.nonfinite(r[name])[0].any()) and bool(nf.nonfinite(r[name])[1, :dh].all())
    assert not bool(nf.nonfinite(r["dkv"])[:nf.POOL_N].any()) and not bool(nf.nonfinite(r["probs"])[:nf.POOL_H].any())


@pytest.mark.parametrize("dtype", nf.GATE_DTYPES, ids=lambda d: kr.DT_NAME[d])
def test_gate_mul_reference_conditions(dtype):
    for n in nf.gate_sizes(dtype):
        conditions(f"gate_mul {kr.DT_NAME[dtype]} n={n}", nf.gate_ref, nf.gate_inputs(dtype, n), nf.gate_sites(n))


@pytest.mark.parametrize("shape", nf.L2_SHAPES, ids=str)
def test_l2norm_tmean_reference_conditions(shape):
    B, T, D = shape
    conditions(f"l2norm_tmean {shape}", nf.l2_ref(B, T), nf.l2_inputs(B, T, D), nf.l2_sites(B, T, D))


@pytest.mark.parametrize("accumulate", [0, 1])
def test_sums_and_copies_reference_conditions(accumulate):
    for dtype in nf.SUM_DTYPES:
        for M, N in nf.COLSUM_SHAPES:
            conditions(f"colsum {kr.DT_NAME[dtype]} {M}x{N}", nf.colsum_ref, nf.colsum_inputs(dtype, M, N, accumulate),
                       nf.colsum_sites(M, N))
    for B, n in nf.BATCH_SUM:
        conditions(f"batch_sum {B}x{n}", nf.colsum_ref, nf.batch_sum_inputs(B, n, accumulate), nf.batch_sum_sites(B, n))
    for n in nf.ADD_N:
        conditions(f"add_f32 n={n}", nf.add_ref, nf.add_inputs(n, accumulate), nf.add_sites(n, accumulate))
    for C in nf.SPLIT3_C:
        conditions(f"split3 C={C}", nf.split3_ref, nf.split3_inputs(C), nf.split3_sites(C))


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("dtype", nf.DW_DTYPES, ids=lambda d: kr.DT_NAME[d])
def test_dwconv_reference_conditions(dtype, accumulate):
    for shape in nf.dw_shapes(dtype):
        conditions(f"dwconv3x3 + wgrad {kr.DT_NAME[dtype]} {shape}", nf.dw_ref, nf.dw_inputs(dtype, *shape, accumulate),
                   nf.dw_sites(*shape))
        inp = nf.dw_inputs(dtype, *shape, accumulate)
        torch.testing.assert_close(nf.dw_ref(inp)["dw10"], kr.dwconv_wgrad_ref(inp["x"], inp["dy"], inp["prior"])[0],
                                   rtol=1e-13, atol=1e-13)
    for rows, cols in nf.VECMAT:
        conditions(f"vecmat {rows}x{cols}", nf.vecmat_ref, nf.vecmat_inputs(rows, cols, accumulate),
                   nf.vecmat_sites(rows, cols))


@pytest.mark.parametrize("shape", nf.SEG_SHAPES, ids=str)
def test_seg_loss_reference_conditions(shape):
    """The conditions, the gather reference against the dense one of tests/kernel_ref.py on clean inputs, and its
    granularity: a NaN logit of image 1 reaches only the chunks whose rows read it bilinearly, all of image 1's gradient
    (through the dice sums), and nothing of images 0 and 2."""
    g, S = shape
    inp = nf.seg_inputs(g, S)
    conditions(f"seg_loss {shape}", nf.seg_ref, inp, nf.seg_sites(g, S))
    r = nf.seg_ref(inp)
    dense, _ = kr.seg_loss_fwd_ref(inp["lr"], inp["tgt"])
    torch.testing.assert_close(r["partial"], dense, rtol=1e-12, atol=1e-12)
    ddense, _ = kr.seg_loss_bwd_ref(inp["lr"], inp["tgt"], r["partial"].sum(1).float(), inp["coef"], nf.SEG_EPS)
    torch.testing.assert_close(r["dlogits"], ddense, rtol=1e-5, atol=1e-12)
    r = nf.seg_ref(nf.poison(inp, ("lr", nf.flat((nf.SEG_B, g, g), (1, g - 1, g - 1))), NAN))
    bad = nf.nonfinite(r["partial"])
    assert not bool(bad[0].any()) and not bool(bad[2].any()) and bool(bad[1, -1, :3].all()) and not bool(bad[1, 0].any())
    assert not bool(bad[1, :, 3].any())                                         # sum t does not read the logits
    assert bool(nf.nonfinite(r["dlogits"])[1].all()) and not bool(nf.nonfinite(r["dlogits"])[[0, 2]].any())


@pytest.mark.parametrize("N,dh", nf.ATTN_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("dtype", nf.ATTN_DTYPES, ids=lambda d: kr.DT_NAME[d])
def test_attn_probs_reference_conditions(dtype, N, dh):
    inp = nf.probs_inputs(dtype, N, dh)
    conditions(f"attn_probs {kr.DT_NAME[dtype]} N={N} dh={dh}", nf.probs_ref, inp, nf.probs_sites(inp))
    r = nf.probs_ref(nf.poison(inp, ("lse", nf.flat((2, 2, N), (1, 0, 0))), NAN))
    assert bool(nf.nonfinite(r["full"])[1, 0, 0].all()) and int(nf.nonfinite(r["full"]).sum()) == N
    assert bool(nf.nonfinite(r["head_mean"])[1, 0].all()) and int(nf.nonfinite(r["head_mean"]).sum()) == N


@pytest.mark.parametrize("accumulate", [0, 1])
def test_folds_reference_conditions(accumulate):
    n, n3, (N1, N2) = nf.RP_N, nf.RP3_N, nf.RS_SHAPE
    conditions("reduce_partials", nf.fold_ref((n,)), nf.fold_inputs(nf.RP_NBLK, n, accumulate, (n,)),
               nf.fold_sites(nf.RP_NBLK, n))
    conditions("reduce_partials3", nf.fold_ref((3, n3)), nf.fold_inputs(nf.RP3_NBLK, 3 * n3, accumulate, (3, n3)),
               nf.fold_sites(nf.RP3_NBLK, 3 * n3))
    conditions("reduce_splits", nf.fold_ref((N1, N2)), nf.fold_inputs(nf.RS_SPLITS, N1 * N2, accumulate, (N1, N2)),
               nf.fold_sites(nf.RS_SPLITS, N1 * N2))


def test_weight_casts_reference_conditions():
    for R, C in nf.CAST_PAD_SHAPES:
        conditions(f"cast_pad {R}x{C}", nf.cast_pad_ref(R + 5, C + 3), nf.cast_pad_inputs(R, C), nf.mat_sites("src", R, C))
    conditions("cast_job", nf.cast_job_ref, nf.cast_job_inputs(), nf.cast_job_sites())


@pytest.mark.parametrize("case", nf.IM2COL, ids=str)
def test_im2col_col2im_reference_conditions(case):
    B, H, W, P, _ = case
    inp = nf.im2col_inputs(B, H, W, P)
    conditions(f"im2col {case}", nf.im2col_ref(P, 640), inp, nf.im2col_sites(B, H, W, P))
    conditions(f"col2im {case}", nf.col2im_ref(H, W, P), inp, nf.col2im_sites(B, H, W, P))


@pytest.mark.parametrize("grid", nf.POS_GRIDS, ids=str)
def test_pos_resize_reference_conditions(grid):
    """Also: the scatter reference of the backward against the dense one of tests/kernel_ref.py on clean inputs, and a
    NaN in one output gradient reaches at most sixteen table entries of its channel."""
    inp = nf.pos_inputs(*grid)
    sites = nf.mat_sites("table", grid[0] ** 2, nf.POS_D)
    conditions(f"pos_resize {grid}", nf.pos_fwd_ref(*grid), inp, sites)
    dsites = nf.mat_sites("dout", grid[1] * grid[2], nf.POS_D)
    conditions(f"pos_resize_bwd {grid}", nf.pos_bwd_ref(*grid), inp, dsites)
    dense, _ = kr.pos_resize_bwd_ref(inp["dout"], *grid, inp["prior"])
    torch.testing.assert_close(nf.pos_bwd_ref(*grid)(inp)["dtable"], dense, rtol=1e-12, atol=1e-12)
    bad = nf.nonfinite(nf.pos_bwd_ref(*grid)(nf.poison(inp, dsites[0], NAN))["dtable"])
    assert 1 <= int(bad.sum()) <= 16 and int(bad[:, 0].sum()) == int(bad.sum())


@pytest.mark.parametrize("case", nf.SEG_EX_CASES, ids=str)
def test_seg_loss_ex_reference_conditions(case):
    """The conditions, and the gather reference against tests/seg_loss_ex_ref.py's dense one on clean inputs."""
    import seg_loss_ex_ref as sr
    inp = nf.seg_ex_inputs(*case)
    conditions(f"seg_loss_ex {case}", nf.seg_ex_ref, inp, nf.seg_ex_sites(*case))
    r = nf.seg_ex_ref(inp)
    dense, _ = sr.seg_loss_ex_fwd_ref(inp["lr"], inp["tgt"], terms=nf.SEG_EX_TERMS)
    torch.testing.assert_close(r["partial"], dense, rtol=1e-11, atol=1e-11)
    ddense, _ = sr.seg_loss_ex_bwd_ref(inp["lr"], inp["tgt"], r["partial"].sum(1), inp["coef"], terms=nf.SEG_EX_TERMS,
                                       eps=nf.SEG_EX_EPS, smooth=nf.SEG_EX_EPS)
    torch.testing.assert_close(r["dlogits"], ddense, rtol=1e-9, atol=1e-14)
    bad = nf.nonfinite(nf.seg_ex_ref(nf.poison(inp, nf.seg_ex_sites(*case)[0], NAN))["partial"])
    assert not bool(bad[0].any()) and bool(bad[1, 0, [0, 1, 2, 4, 5, 6, 7]].all()) and not bool(bad[1, :, 3].any())


def test_cast_reference_conditions():
    conditions("cast_f32", nf.cast_ref, nf.cast_inputs(), nf.cast_sites())
