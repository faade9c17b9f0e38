"""The non-finite propagation contract ("Non-finite values") as one generic driver, and the case tables
that tests/test_nonfinite_host.py (references only, CPU) and tests/test_nonfinite_gpu.py (kernels) share.

An op is a runner `run(inputs, poisoned) -> {name: tensor}` (the kernel through the C ABI: the runners of
tests/attn_util.py and tests/op_runners.py, nothing launched from here) and a float64 reference `ref(inputs) ->
{name: tensor}` of the same names and shapes (tests/kernel_ref.py).  `inputs` is a dict of named operands in the
dtype the kernel receives; a poison site is (operand name, flat index), or (operand name, flat index, value names) where a
table had to move one value's case to another element (rule 3 below).  Per site the kernel and the reference run with
NaN, +inf and -inf at that element, and for every output element e:

  rule 1, no swallowing   the reference's e is non-finite           ->  the kernel's e is non-finite (NaN or +-inf, any)
  rule 2, no spreading    the reference's e of the NaN run is finite ->  the kernel's e has the bits of the clean launch
  excused                 non-finite in the NaN run but finite for this +-inf: nothing is asserted

The excused set of a NaN poison has to be empty, and `reference_conditions` checks that on the reference alone, with
a dependency found without any table: an element depends on the site if a FINITE change of the site's value changes
its float64 reference.  Every such element has to be non-finite in the NaN run.  The same function checks that a +-inf
poison makes nothing non-finite that NaN leaves finite (0 * inf would: the clean inputs hold no exact zero, `nonzero`)
and that at most half of a site's dependent elements are excused.
"""
import math

import torch

import kernel_ref as kr
from kernel_ref import BF16, BF16X3, F16, F32

NAN, INF = float("nan"), float("inf")
VALUES = (("nan", NAN), ("+inf", INF), ("-inf", -INF))
MAX_EXCUSED_SHARE = 0.5


# ---------------------------------------------------------------------------------------------------------------
# small helpers
# ---------------------------------------------------------------------------------------------------------------
def nonzero(t):
    """t with every exact zero replaced by one (0 * inf would change the class of the reference)."""
    t = t.clone()
    t[t == 0] = 1
    return t


def poison(inputs, site, value):
    """A shallow copy of `inputs` whose operand site[0] is a clone with `value` at flat index site[1]."""
    name, flat = site[:2]
    out = dict(inputs)
    t = inputs[name].clone().contiguous()
    t.view(-1)[flat] = value
    out[name] = t
    return out


def perturbed(inputs, site):
    """`inputs` with a finite, different value at the site: far enough to move a bf16 and to change every sum it
    enters (x -> 1.25 x + 0.5, or -0.75 where that is x itself)."""
    name, flat = site[:2]
    x = inputs[name].view(-1)[flat].double().item()
    y = 1.25 * x + 0.5
    if torch.tensor(y).to(inputs[name].dtype).double().item() == x:
        y = -0.75
    return poison(inputs, site, y)


def site_values(site):
    """The (name, value) pairs a site is poisoned with: all of VALUES unless the site names its own."""
    return VALUES if len(site) == 2 else tuple(nv for nv in VALUES if nv[0] in site[2])


def site_name(inputs, site):
    name, flat = site[:2]
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(flat), inputs[name].shape))
    return f"{name}{list(idx)}"


def bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def hex_of(t, i):
    n = t.element_size()
    return f"0x{int(bits(t).flatten()[i].item()) & ((1 << (8 * n)) - 1):0{2 * n}x}"


def first_index(mask):
    i = int(mask.flatten().nonzero()[0].item())
    return i, tuple(int(v) for v in torch.unravel_index(torch.tensor(i), mask.shape))


def nonfinite(t):
    return ~torch.isfinite(t.double())


# ---------------------------------------------------------------------------------------------------------------
# the rules, on masks
# ---------------------------------------------------------------------------------------------------------------
def apply_rules(what, clean, got, dep, must, ref_v=None, bound=None):
    """Rules 1 and 2 for one output of one (site, value) run.  clean / got: the kernel's output of the clean and of the
    poisoned launch; dep: non-finite in the reference's NaN run; must: non-finite in the reference's run of this value.
    With `bound` (an op whose summation order is not fixed: atomics) the independent elements are held to
    |got - ref_v| <= bound, not to the clean launch's bits.  Returns (number excused, number dependent)."""
    assert clean.shape == got.shape == dep.shape == must.shape, \
        f"{what}: shapes {tuple(clean.shape)} {tuple(got.shape)} {tuple(dep.shape)} {tuple(must.shape)}"
    swallowed = must & torch.isfinite(got.double())
    if bool(swallowed.any()):
        i, idx = first_index(swallowed)
        raise AssertionError(f"{what}: rule 1 (no swallowing): {int(swallowed.sum())} elements are finite where the "
                             f"float64 reference is not; first at {idx}: kernel {got.flatten()[i].item():.9g} "
                             f"(bits {hex_of(got, i)}), clean launch {clean.flatten()[i].item():.9g} "
                             f"(bits {hex_of(clean, i)})")
    indep = ~dep
    if bound is None:
        spread = indep & (bits(got) != bits(clean))
    else:
        spread = indep & ~((got.double() - ref_v.double()).abs() <= bound.double())
    if bool(spread.any()):
        i, idx = first_index(spread)
        how = "differ from the clean launch" if bound is None else "are outside the op's float64 bound"
        raise AssertionError(f"{what}: rule 2 (no spreading): {int(spread.sum())} elements that do not depend on the "
                             f"poisoned element {how}; first at {idx}: kernel {got.flatten()[i].item():.9g} "
                             f"(bits {hex_of(got, i)}), clean launch {clean.flatten()[i].item():.9g} "
                             f"(bits {hex_of(clean, i)})")
    return int((dep & ~must).sum()), int(dep.sum())


def reference_conditions(op, ref, inputs, site, ref_clean=None):
    """The conditions of the test that involve the reference alone, for one site.  Returns (ref_by_value, shares):
    the reference outputs per value name, and the excused share (excused / dependent over all outputs) per value name."""
    where = f"{op} {site_name(inputs, site)}"
    ref_clean = ref(inputs) if ref_clean is None else ref_clean
    for name, t in ref_clean.items():
        assert bool(torch.isfinite(t).all()), f"{op}: the clean reference of {name} is not finite"
    moved = ref(perturbed(inputs, site))
    refs = {vn: ref(poison(inputs, site, v)) for vn, v in VALUES if vn == "nan" or (vn, v) in site_values(site)}
    shares = {}
    for vn in refs:
        exc = dep_n = 0
        for name, t_nan in refs["nan"].items():
            dep = nonfinite(t_nan)
            if vn == "nan":
                truly = moved[name] != ref_clean[name]
                miss = truly & ~dep
                if bool(miss.any()):
                    _, idx = first_index(miss)
                    raise AssertionError(f"{where} NaN {name}: the excused set of a NaN poison is not empty: element "
                                         f"{idx} changes with a finite change of the site, but the reference's NaN run "
                                         f"leaves it finite ({int(miss.sum())} such elements)")
            else:
                must = nonfinite(refs[vn][name])
                stray = must & ~dep
                if bool(stray.any()):
                    _, idx = first_index(stray)
                    raise AssertionError(f"{where} {vn} {name}: element {idx} is non-finite in the reference although "
                                         f"the NaN run leaves it finite (0 * inf in the clean inputs?)")
                exc += int((dep & ~must).sum())
            dep_n += int(dep.sum())
        assert dep_n > 0, f"{where}: no output depends on the site"
        shares[vn] = exc / dep_n
        assert shares[vn] <= MAX_EXCUSED_SHARE, \
            f"{where} {vn}: {exc} of {dep_n} dependent elements are excused (more than half): choose another site"
    return refs, shares


class Stats:
    """(site, value) cases and the largest excused share of an op, printed by the tests (pytest -s shows them)."""

    def __init__(self, op):
        self.op, self.cases, self.worst, self.worst_at = op, 0, 0.0, ""

    def add(self, where, share):
        self.cases += 1
        if share > self.worst:
            self.worst, self.worst_at = share, where

    def line(self):
        at = f" at {self.worst_at}" if self.worst_at else ""
        return f"[nonfinite] {self.op}: {self.cases} (site, value) cases, largest excused share {self.worst:.3f}{at}"


def drive(op, run, ref, inputs, sites, bounds=None, to_ref=None):
    """Runs the kernel once clean, then per site and per value the kernel and the reference, and applies rules 1 to 3.
    run(inputs, poisoned) -> {name: tensor}; ref(inputs) -> {name: float64 tensor}; to_ref moves the inputs to where
    the reference runs (default: as they are); bounds(poisoned inputs) -> {name: bound} switches rule 2 of the named
    outputs from bit equality to the op's float64 bound."""
    to_ref = to_ref or (lambda d: d)
    st = Stats(op)
    clean = {k: v.clone() for k, v in run(inputs, False).items()}
    rin = to_ref(inputs)
    ref_clean = ref(rin)
    assert set(ref_clean) == set(clean), f"{op}: outputs {sorted(clean)} vs reference {sorted(ref_clean)}"
    for site in sites:
        refs, shares = reference_conditions(op, ref, rin, site, ref_clean)       # before any poisoned launch
        for vn, v in site_values(site):
            got = run(poison(inputs, site, v), True)
            bnd = bounds(poison(rin, site, v)) if bounds else {}
            where = f"{op} {site_name(inputs, site)}={vn}"
            for name in clean:
                dep, must = nonfinite(refs["nan"][name]), nonfinite(refs[vn][name])
                apply_rules(f"{where} -> {name}", clean[name], got[name], dep.to(got[name].device),
                            must.to(got[name].device), refs[vn][name].to(got[name].device),
                            bnd.get(name))
            st.add(f"{site_name(inputs, site)}={vn}", shares[vn])
    print(st.line())
    return st


# ---------------------------------------------------------------------------------------------------------------
# case tables: inputs (CPU, in the kernel's dtype), sites and the float64 reference of every op
# ---------------------------------------------------------------------------------------------------------------
def flat(shape, idx):
    f = 0
    for n, i in zip(shape, idx):
        assert 0 <= i < n
        f = f * n + i
    return f


# ---- attention ---------------------------------------------------------------------------------------------------
ATTN_DTYPES = [BF16, F16, F32, BF16X3]
ATTN_SHAPES = [(33, 8), (130, 72)]           # B = 2, H = 2; see the issue's reasons in tests/test_nonfinite_gpu.py
ATTN_B, ATTN_H = 2, 2
ATTN_HEAD = (1, 0)                           # the poisoned (b, h)


def attn_inputs(dtype, N, dh):
    q, k, v, do = kr.attn_inputs("gauss", ATTN_B, ATTN_H, N, dh, kr.TORCH_DT[dtype], seed=N + dh)
    return dict(q=nonzero(q), k=nonzero(k), v=nonzero(v), dout=nonzero(do))


def attn_positions(N, dh):
    return [(0, 0), (N - 1, dh - 1)] + ([(64, dh - 1)] if N == 130 else [])


def attn_sites(inp, operands=("q", "k", "v", "dout")):
    """Every operand at every position of `attn_positions`.  One kind of case cannot stay where the table puts it: with
    k[j, c] = +-inf the score of query i is +-inf by the sign of q[i, c], and a query whose score is -inf has probability 0
    there and an entirely finite row of O, lse and dQ; dV is finite outside row j too (P is NaN at key j and 0 elsewhere in
    the other rows).  So one of +inf / -inf always has more than half of the dependent set excused at the same element
    (N = 33: 1089 dependent, 272 + 17 per query with a +inf score non-finite).  That value's case moves to the nearest
    column of the same key where the queries with a +inf score are a majority of at least N / 2 + 1."""
    shape = tuple(inp["q"].shape)
    N, dh = shape[2:]
    sites = []
    for o in operands:
        for row, col in attn_positions(N, dh):
            if o != "k":
                sites.append((o, flat(shape, ATTN_HEAD + (row, col))))
                continue
            qs = inp["q"][ATTN_HEAD].double()
            at = {}
            for vn, v in VALUES:
                fav = [int(((qs[:, c] * v) > 0).sum()) if vn != "nan" else N for c in range(dh)]
                good = [c for c in range(dh) if fav[c] >= N // 2 + 1]
                at.setdefault(min(good, key=lambda c: (abs(c - col), c)), []).append(vn)
            sites += [("k", flat(shape, ATTN_HEAD + (row, c)), tuple(vns)) for c, vns in sorted(at.items())]
    return sites


def attn_ref(inp):
    r = kr.attn_ref(inp["q"], inp["k"], inp["v"], inp["dout"])
    return dict(O=r["O"], lse=r["lse"], dQ=r["dQ"], dK=r["dK"], dV=r["dV"])


# ---- LayerNorm ---------------------------------------------------------------------------------------------------
LN_M = 5
LN_D = [4, 516, 1152]
LN_DTYPES = [F32, BF16, F16]
LN_EPS = 1e-6


def ln_inputs(D, dtype, dres):
    """x, gamma, beta fp32; dy in the forward's output dtype (as the encoder's backward receives it); dres fp32 or None."""
    g = torch.Generator(device="cpu").manual_seed(D)
    rn = lambda *s: torch.randn(*s, generator=g)
    inp = dict(x=nonzero(rn(LN_M, D) * 2 + 0.3), gamma=nonzero(rn(D) * 0.2 + 1), beta=rn(D) * 0.1,
               dy=nonzero(rn(LN_M, D).to(kr.TORCH_DT[dtype])))
    inp["dres"] = rn(LN_M, D) if dres else None
    return inp


def ln_sites(D):
    s = [(o, flat((LN_M, D), (r, c))) for o in ("x", "dy") for r in (0, LN_M - 1) for c in (0, D - 1)]
    return s + [("gamma", 0), ("gamma", D - 1)]


def ln_ref(inp):
    (y, _), (mu, _), (rs, _) = kr.ln_fwd_ref(inp["x"], inp["gamma"], inp["beta"], LN_EPS, 0.0)
    (dx, _, _), (dg, _), (db, _) = kr.ln_bwd_ref(inp["dy"], inp["x"], mu, rs, inp["gamma"], inp["dres"], 0.0)
    return dict(y=y, mean=mu, rstd=rs, dx=dx, dx_lp=dx, dgamma=dg, dbeta=db)


# ---- NT GEMM -----------------------------------------------------------------------------------------------------
NT_DTYPES = [BF16, F16, F32, BF16X3]
NT_M = [333, 2333]
NT_N, NT_K = 264, 72
NT_EPIS = [0, 1, 2, 4, 5, 6]
NT_POS_ROWS = 37
NT_WIDE = (2333, 1152, 72, 0)              # M, N, K, epilogue: the encoder's width, plain store -> the 384 x 192 tile


def nt_inputs(dtype, M, epi, N=NT_N, K=NT_K):
    """A [M, K], B [N, K] in the operand dtype, bias fp32 (none for the GELU-backward epilogue 4), and what the epilogue
    reads: res (2, fp32), aux (4, the saved GELU operand, in the output dtype), pos (5, fp32)."""
    g = torch.Generator(device="cpu").manual_seed(M + epi)
    rn = lambda *s: torch.randn(*s, generator=g)
    tdt = kr.TORCH_DT[dtype]
    inp = dict(A=nonzero(rn(M, K).to(tdt)), B=nonzero((rn(N, K) / math.sqrt(K)).to(tdt)))
    if epi != 4:
        inp["bias"] = rn(N)
    if epi == 2:
        inp["res"] = rn(M, N)
    if epi == 4:
        inp["aux"] = nonzero((rn(M, N) * 1.5).to(tdt))
    if epi == 5:
        inp["pos"] = rn(NT_POS_ROWS, N)
    return inp


def nt_sites(M, epi, N=NT_N, K=NT_K):
    """A[i, k], B[j, k] with k in {0, K - 1} (K - 1 = 71 lies in the partial K step) and i, j in the first and in the last
    (partial) tile; the bias, residual, saved operand and position element that the epilogue reads."""
    rows, cols, ks = (0, M - 1), (0, N - 1), (0, K - 1)
    s = [("A", flat((M, K), (i, k))) for i in rows for k in ks]
    s += [("B", flat((N, K), (j, k))) for j in cols for k in ks]
    if epi != 4:
        s += [("bias", j) for j in cols]
    if epi == 2:
        s += [("res", flat((M, N), (0, 0))), ("res", flat((M, N), (M - 1, N - 1)))]
    if epi == 4:
        s += [("aux", flat((M, N), (0, 0))), ("aux", flat((M, N), (M - 1, N - 1)))]
    if epi == 5:
        s += [("pos", 0), ("pos", flat((NT_POS_ROWS, N), ((M - 1) % NT_POS_ROWS, N - 1)))]
    return s


def nt_ref(epi):
    def ref(inp):
        r = inp["A"].double() @ inp["B"].double().t()
        M = r.shape[0]
        if "bias" in inp:
            r = r + inp["bias"].double()[None, :]
        if epi == 2:
            r = r + inp["res"].double()
        if epi == 5:
            r = r + inp["pos"].double()[torch.arange(M, device=r.device) % NT_POS_ROWS]
        if epi == 4:
            return dict(out=r * kr.gelu_grad64(inp["aux"]))
        if epi == 1:
            return dict(out=r, out2=kr.gelu64(r))
        return dict(out=r)
    return ref


QKV_SHAPES = [(2, 50, 4, 40), (7, 300, 4, 40)]       # batch, tokens, heads, hd: M = 100 (small tiles) and 2100 (256-row tiles)


def qkv_inputs(dtype, batch, tokens, heads, hd):
    g = torch.Generator(device="cpu").manual_seed(batch + hd)
    rn = lambda *s: torch.randn(*s, generator=g)
    tdt, D = kr.TORCH_DT[dtype], heads * hd
    return dict(A=nonzero(rn(batch * tokens, D).to(tdt)), B=nonzero((rn(3 * D, D) / math.sqrt(D)).to(tdt)), bias=rn(3 * D))


def qkv_sites(batch, tokens, heads, hd):
    M, D = batch * tokens, heads * hd
    return [("A", 0), ("A", flat((M, D), (M - 1, D - 1))), ("B", 0), ("B", flat((3 * D, D), (3 * D - 1, D - 1))),
            ("bias", 0), ("bias", 3 * D - 1)]


def qkv_ref(batch, tokens, heads, hd):
    def ref(inp):
        r = inp["A"].double() @ inp["B"].double().t() + inp["bias"].double()[None, :]
        return dict(qkv=r.view(batch, tokens, 3, heads, hd).permute(2, 0, 3, 1, 4))
    return ref


# ---- TN GEMM -----------------------------------------------------------------------------------------------------
TN_DTYPES = [BF16, F16]
TN_N = 512
# name, Mred, N2, splits, scratch bytes (None: sgl_op_gemm_tn), whether the summation order is fixed (rule 2 by bits)
TN_ROUTES = [("small_tile_one_split", 2047, 512, 1, None, True),
             ("small_tile_three_splits_atomics", 2047, 512, 3, None, False),
             # Mred >= 2048 with N1, N2 >= 512: gemm_tn_mfma (csrc/gemm_bf16.hip) ignores `splits` and takes the plan of
             # tn_plan (csrc/kernels.h), which splits the reduction to fill the chip and adds with atomics without scratch
             # (a static_assert next to the encoder's plans in csrc/encoder.hip pins that this shape is split)
             ("tn256_own_splits_atomics", 2048, 512, 1, None, False),
             ("tn256_ws_slabs", 2048, 512, 1, 64 << 20, True)]
TN_FALLBACKS = [("ws_too_small_atomics", 2048, 512, 1, 4096, False),
                ("ws_n2_mod4_atomics", 2048, 514, 1, 64 << 20, False)]


def tn_inputs(dtype, Mred, N2, accumulate, N1=TN_N):
    g = torch.Generator(device="cpu").manual_seed(Mred + N2)
    rn = lambda *s: torch.randn(*s, generator=g)
    tdt = kr.TORCH_DT[dtype]
    inp = dict(A=nonzero(rn(Mred, N1).to(tdt)), B=nonzero(rn(Mred, N2).to(tdt)))
    inp["prior"] = rn(N1, N2) * 3 if accumulate else None
    return inp


def tn_sites(Mred, N2, N1=TN_N):
    """A[m, i] poisons row i of dW, B[m, j] column j; m = Mred - 1 is a row of the last split."""
    return [("A", flat((Mred, N1), (Mred - 1, 0))), ("A", flat((Mred, N1), (0, N1 - 1))),
            ("B", flat((Mred, N2), (Mred - 1, N2 - 1))), ("B", flat((Mred, N2), (0, 0)))]


def tn_ref(inp):
    return dict(out=kr.gemm_tn_ref(inp["A"], inp["B"], inp["A"].shape[0], inp["prior"])[0])


def tn_bounds(inp):
    return dict(out=kr.gemm_tn_ref(inp["A"], inp["B"], inp["A"].shape[0], inp["prior"])[1])


# ---- LayerNorm -> MX operand, and quantize -> MX GEMM --------------------------------------------------------
LN_MX_D = [8, 520, 1152]                    # sgl_op_layernorm_fwd_mx takes D % 8 == 0 only: the neighbours of LN_D's 4 and 516


def mx_kpad(K):
    return (K + 127) // 128 * 128


def ln_mx_inputs(D):
    inp = ln_inputs(D, F32, False)
    return dict(x=inp["x"], gamma=inp["gamma"], beta=inp["beta"])


def ln_mx_sites(D):
    return [s for s in ln_sites(D) if s[0] != "dy"]


def ln_mx_ref(inp):
    """The values the MX operand stands for: float64 LayerNorm, quantised by the reference quantiser (a block that holds
    an inf or a NaN is NaN as a whole: scale byte 0xFF) and dequantised; the columns D..Kp are zeros."""
    import mx_ref
    (y, _), _, _ = kr.ln_fwd_ref(inp["x"], inp["gamma"], inp["beta"], LN_EPS, 0.0)
    q, s = mx_ref.quantize(y, Kp=mx_kpad(y.shape[1]))
    return dict(deq=mx_ref.dequantize(q, s))


MX_M, MX_N, MX_K = 333, 264, 72


def mx_gemm_inputs():
    g = torch.Generator(device="cpu").manual_seed(5)
    rn = lambda *s: torch.randn(*s, generator=g)
    return dict(x=nonzero(rn(MX_M, MX_K)), w=nonzero(rn(MX_N, MX_K) / math.sqrt(MX_K)), bias=rn(MX_N), res=rn(MX_M, MX_N))


def mx_gemm_sites():
    return [("x", flat((MX_M, MX_K), ik)) for ik in ((0, 0), (MX_M - 1, MX_K - 1), (200, 40))]


def mx_gemm_ref(inp):
    """res + quantised(x) . quantised(w)^T + bias in float64 on the values the reference quantiser gives."""
    import mx_ref
    a = mx_ref.dequantize(*mx_ref.quantize(inp["x"]))
    b = mx_ref.dequantize(*mx_ref.quantize(inp["w"]))
    return dict(out=inp["res"].double() + a @ b.t() + inp["bias"].double())


# ---- pooling-head attention ---------------------------------------------------------------------------------------
POOL_B, POOL_H, POOL_N = 2, 2, 100
POOL_DTYPES = [F32, BF16, F16]
POOL_DIMS = [(8, 16), (88, 96)]             # (head_dim, head_dim_pad): the first and the last entry of the edge tests' POOL_DIMS


def pool_inputs(dtype, dh, DP):
    """q [H * dh] fp32 (one query per head, shared by the images), K, V head-major [B, H, N, DP] with zero pad columns,
    dout [B, H * dh] fp32."""
    q, K, V, do = kr.pool_inputs("gauss", POOL_B, POOL_H, POOL_N, dh, DP, kr.TORCH_DT[dtype], seed=dh)
    K, V = K.clone(), V.clone()
    K[..., :dh], V[..., :dh] = nonzero(K[..., :dh]), nonzero(V[..., :dh])
    q = nonzero(q)
    q[0], q[1], q[dh - 2], q[dh - 1] = q[0].abs(), -q[1].abs(), q[dh - 2].abs(), -q[dh - 1].abs()   # both signs next to
    return dict(q=q, K=K, V=V, dout=nonzero(do))                                                   # either K site


def pool_sites(inp, dh):
    """q at its first and last element; K, V at the first and the last token of image 1, head 0; dout of image 1.
    A K element at +-inf makes that token's score +-inf by the sign of q[c]: at -inf its probability is 0 and nothing
    at all is non-finite, so each of the two values goes to the nearest column where the score is +inf."""
    ks = tuple(inp["K"].shape)
    s = [("q", 0), ("q", inp["q"].numel() - 1)]
    for n, col in ((0, 0), (POOL_N - 1, dh - 1)):
        at = {}
        for vn, v in VALUES:
            good = [c for c in range(dh) if vn == "nan" or inp["q"][c].item() * v > 0]       # head 0: q[0:dh]
            at.setdefault(min(good, key=lambda c: (abs(c - col), c)), []).append(vn)
        s += [("K", flat(ks, (1, 0, n, c)), tuple(vns)) for c, vns in sorted(at.items())]
        s.append(("V", flat(ks, (1, 0, n, col))))
    ds = tuple(inp["dout"].shape)
    return s + [("dout", flat(ds, (1, 0))), ("dout", flat(ds, (1, ds[1] - 1)))]


def pool_ref(dh):
    def ref(inp):
        K64, V64 = inp["K"].double()[..., :dh], inp["V"].double()[..., :dh]
        B, H, N, _ = K64.shape
        q64, dO = inp["q"].double().view(H, dh), inp["dout"].double().view(B, H, dh)
        scale = dh ** -0.5
        Pr = torch.softmax(torch.einsum("hd,bhnd->bhn", q64, K64) * scale, -1)
        out = torch.einsum("bhn,bhnd->bhd", Pr, V64)
        dp = torch.einsum("bhd,bhnd->bhn", dO, V64)
        ds = Pr * (dp - (Pr * dp).sum(-1, keepdim=True)) * scale
        dK = ds[..., None] * q64[None, :, None, :]
        dV = Pr[..., None] * dO[:, :, None, :]
        tok = lambda t: t.permute(0, 2, 1, 3).reshape(B * N, H * dh)
        return dict(out=out.reshape(B, H * dh), probs=Pr.reshape(B * H, N), dkv=torch.cat([tok(dK), tok(dV)], 1),
                    dq=torch.einsum("bhn,bhnd->bhd", ds, K64).reshape(B, H * dh))
    return ref


# ---- gate_mul, l2norm_tmean -----------------------------------------------------------------------------------------
GATE_DTYPES = [F32, BF16]


def gate_sizes(dtype):
    nv = kr.NV[dtype]
    return [nv, 256 * nv * 3 + nv]          # one vector; three blocks and one vector


def gate_inputs(dtype, n):
    g = torch.Generator(device="cpu").manual_seed(n)
    rn = lambda *s: torch.randn(*s, generator=g)
    tdt = kr.TORCH_DT[dtype]
    return dict(gate=nonzero((rn(n) * 2).to(tdt)), x=nonzero(rn(n).to(tdt)), dy=nonzero(rn(n).to(tdt)))


def gate_sites(n):
    """First, last and one element of the last vector.  A gate at +-inf has sigmoid 1 or 0 exactly: y, dg and dx are all
    finite (x, 0, dy or 0, 0, 0), the whole dependent set is excused at every element, so the gate is poisoned with NaN
    only."""
    pos = sorted({0, n - 1, n - 3})
    return [("gate", i, ("nan",)) for i in pos] + [(o, i) for o in ("x", "dy") for i in pos]


def gate_ref(inp):
    s = torch.sigmoid(inp["gate"].double())
    x, dy = inp["x"].double(), inp["dy"].double()
    return dict(y=s * x, dg=dy * x * (s * (1 - s)), dx=dy * s)


L2_SHAPES = [(3, 4, 100), (2, 3, 257)]      # two of the edge tests' smallest with more than one frame


def l2_inputs(B, T, D):
    g = torch.Generator(device="cpu").manual_seed(D)
    return dict(f=nonzero(torch.randn(B * T, D, generator=g) * 3), dout=nonzero(torch.randn(B, D, generator=g)))


def l2_sites(B, T, D):
    return [("f", 0), ("f", B * T * D - 1), ("f", flat((B * T, D), (T, D - 3))), ("dout", 0), ("dout", B * D - 1)]


def l2_ref(B, T):
    def ref(inp):
        (out, _), (inv, _) = kr.l2norm_tmean_fwd_ref(inp["f"], B, T)
        df, _ = kr.l2norm_tmean_bwd_ref(inp["f"], inv, inp["dout"], B, T)
        return dict(out=out, inv_norm=inv, df=df)
    return ref


# ---- depthwise 3x3 and its weight gradient ------------------------------------------------------------------------
DW_DTYPES = [F32, BF16]


def dw_shapes(dtype):
    return [(2, 1, 7, kr.NV[dtype]), (2, 5, 7, 64)]       # B, gh, gw, E: one channel vector on a one-row grid; 64 channels


def dw_inputs(dtype, B, gh, gw, E, accumulate):
    g = torch.Generator(device="cpu").manual_seed(gh * 8 + gw + E)
    rn = lambda *s: torch.randn(*s, generator=g)
    tdt = kr.TORCH_DT[dtype]
    inp = dict(x=nonzero(rn(B, gh, gw, E).to(tdt)), dy=nonzero(rn(B, gh, gw, E).to(tdt)), w9=nonzero(rn(9, E)), bias=rn(E))
    inp["prior"] = rn(10, E) if accumulate else None
    return inp


def dw_sites(B, gh, gw, E):
    """x and dy at the first pixel, the last pixel of image 1 and an inner one; a bias element; the first tap (which a
    pixel of the first row or column does not have: those keep their bits) and the centre tap of one channel."""
    sh = (B, gh, gw, E)
    pos = [(0, 0, 0, 0), (B - 1, gh - 1, gw - 1, E - 1), (B - 1, gh // 2, gw // 2, E - 3)]
    return [(o, flat(sh, i)) for o in ("x", "dy") for i in pos] + [("bias", E - 1), ("w9", flat((9, E), (4, 0)))] + \
        ([("w9", flat((9, E), (0, E - 1)))] if gh > 1 else [])          # a one-row grid never reads the upper taps


def dw_ref(inp):
    """y and the weight gradient written out with the out-of-range taps LEFT OUT (kernel_ref's references multiply them
    by a zero padding, and 0 * NaN would poison taps that a border pixel does not have)."""
    x64, d64, w64 = inp["x"].double(), inp["dy"].double(), inp["w9"].double()
    E = x64.shape[-1]
    ones = torch.ones_like(x64[..., :1])
    y = torch.zeros_like(x64) + inp["bias"].double()
    for k in range(9):
        live = kr._shift(ones, k // 3, k % 3) != 0
        y = y + torch.where(live, w64[k] * kr._shift(x64, k // 3, k % 3), torch.zeros_like(x64))
    rows = []
    for k in range(9):
        live = kr._shift(ones, k // 3, k % 3) != 0
        t = torch.where(live, kr._shift(x64, k // 3, k % 3) * d64, torch.zeros_like(d64))
        rows.append(t.reshape(-1, E).sum(0))
    rows.append(d64.reshape(-1, E).sum(0))
    dw = torch.stack(rows)
    return dict(y=y, dw10=dw if inp["prior"] is None else dw + inp["prior"].double())


# ---- seg_loss -----------------------------------------------------------------------------------------------------
SEG_SHAPES = [(3, 42), (4, 56)]             # two of the edge tests' smallest; scale 1 / 14: no bilinear weight is exactly zero
SEG_B, SEG_EPS = 3, 1e-6                    # away from the clamped border, so no tap is multiplied by 0


def seg_inputs(g, S):
    gen_ = torch.Generator(device="cpu").manual_seed(g * 1000 + S)
    lr = nonzero(torch.randn(SEG_B, g, g, generator=gen_) * 2.5)
    tgt = (torch.rand(SEG_B, S, S, generator=gen_) < 0.3).float()
    coef = torch.tensor([[1.7e-5, -0.21], [0.9e-5, -0.4], [2.0e-5, -0.3]])
    return dict(lr=lr, tgt=tgt, coef=coef)


def seg_sites(g, S):
    """A logit of image 1 at the first, the last and an inner position, and a target pixel of image 1.  A logit at +-inf
    saturates the sigmoid exactly: p, p t and p (1 - p) are finite, so are the dice sums and the whole gradient, and only
    the bce sums are not; more than half is excused wherever it sits, so the logits are poisoned with NaN only."""
    nan = ("nan",)
    return [("lr", flat((SEG_B, g, g), (1, 0, 0)), nan), ("lr", flat((SEG_B, g, g), (1, g - 1, g - 1)), nan),
            ("lr", flat((SEG_B, g, g), (1, g // 2, g - 2)), nan), ("tgt", flat((SEG_B, S, S), (1, S // 2, S - 3)))]


def seg_gather(L, S):
    """The bilinear upsampling of L [B, g, g] (float64) to S x S by GATHERS, with the kernel's fp32 scale: returns z, the
    transposed scatter dz [B, S, S] -> [B, g, g] (taps of weight 0 and the doubled tap of a clamped border left out), and
    `same` [S - 1]: outputs k and k + 1 have the same interpolation row."""
    B, g = L.shape[0], L.shape[-1]
    dev = L.device
    scale = (torch.tensor(float(g), dtype=torch.float32) / torch.tensor(float(S), dtype=torch.float32)).double().item()
    i = torch.arange(S, dtype=torch.float64, device=dev)
    s = (scale * (i + 0.5) - 0.5).clamp_min(0.0)
    i0 = s.floor().clamp_max(g - 1).long()
    i1 = (i0 + 1).clamp_max(g - 1)
    w = s - i0.double()
    same = i0 == i1                                       # the clamped border: one tap, read once
    wx, wy = w[None, None, :], w[None, :, None]

    def lerp(a, b, wt, eq):
        return torch.where(eq, a, a * (1 - wt) + b * wt)
    top = lerp(L[:, i0][:, :, i0], L[:, i0][:, :, i1], wx, same[None, None, :])
    bot = lerp(L[:, i1][:, :, i0], L[:, i1][:, :, i1], wx, same[None, None, :])
    z = lerp(top, bot, wy, same[None, :, None])
    one = torch.ones_like(w)
    w0, w1 = torch.where(same, one, 1 - w), torch.where(same, 0 * one, w)

    def scatter(dz):
        dl = torch.zeros(B, g, g, dtype=torch.float64, device=dev)
        for iy, wy_ in ((i0, w0), (i1, w1)):
            for ix, wx_ in ((i0, w0), (i1, w1)):
                live = ((wy_ != 0)[:, None] & (wx_ != 0)[None, :])[None]
                contrib = torch.where(live, dz * wy_[None, :, None] * wx_[None, None, :], torch.zeros_like(dz))
                dl.view(B, g * g).index_add_(1, (iy[:, None] * g + ix[None, :]).reshape(-1), contrib.reshape(B, -1))
        return dl
    row_same = (i0[1:] == i0[:-1]) & (i1[1:] == i1[:-1]) & ((w[1:] == w[:-1]) | same[1:])
    return z, scatter, row_same


SEG_EX_CASES = [(2, 3, 42), (2, 5, 37)]     # B, g, S: the two smallest of tests/seg_loss_ex_ref.py
SEG_EX_TERMS, SEG_EX_EPS = 7, 1e-6


def seg_ex_inputs(B, g, S):
    import seg_loss_ex_ref as sr
    lr, tgt, coef = sr.inputs(B, g, S, 0)
    return dict(lr=nonzero(lr), tgt=tgt, coef=coef)


def seg_ex_sites(B, g, S):
    """A logit of image 1 at the first, the last and an inner position, NaN only (see seg_sites).  The targets are left
    alone: the boundary weight is made of comparisons on a 3 x 3 box sum of the mask, which drop a NaN in float64 too."""
    return [("lr", flat((B, g, g), (1,) + ij), ("nan",)) for ij in ((0, 0), (g - 1, g - 1), (g // 2, g - 2))]


def seg_ex_ref(inp):
    """seg_loss_ex forward and backward in float64, CPU: the per-pixel terms and dz of tests/seg_loss_ex_ref.py on a z
    that is GATHERED (its own is a dense matrix product), and the scatter of seg_gather.  partial [B, chunks, 8] and
    dlogits_lr from the sums of those partials."""
    import seg_loss_ex_ref as sr
    L, t = inp["lr"].double().cpu(), inp["tgt"].double().cpu()
    z, scatter, same = seg_gather(L, t.shape[-1])
    p = torch.sigmoid(z)
    bce = z.clamp_min(0) - z * t + torch.log1p(torch.exp(-z.abs()))
    a = kr._f32c(sr.ALPHA)
    q = p + t - 2 * p * t
    at = a * t + (1 - a) * (1 - t)
    bs = sr.box_sum(t)
    wb = 1 + 3 * ((bs > 0).double() - (bs == 9).double())
    zero = torch.zeros_like(p)
    # plain differences: two pixels with the same interpolation row have the same z to the bit, so a clean pair gives
    # exactly 0 without being told to, and a pair of NaNs gives NaN, as in the kernel
    dx, dy = p[:, :, 1:] - p[:, :, :-1], p[:, 1:, :] - p[:, :-1, :]
    r = dict(p=p, t=t, bce=bce, q=q, at=at, focal=at * q * q * bce, wb=wb, bnd=wb * bce, dx=dx, dy=dy, same=same,
             ep=zero, ebce=zero, eq=zero, eat=zero, efocal=zero, ebnd=zero, edx=zero[:, :, 1:], edy=zero[:, 1:, :],
             amb_x=zero[:, :, 1:].bool(), amb_y=zero[:, 1:, :].bool())
    partial, _ = sr.seg_loss_ex_fwd_ref(L, t, terms=SEG_EX_TERMS, r=r)
    dz, _ = sr.pixel_grad_ref(r, partial.sum(1), inp["coef"].cpu(), SEG_EX_TERMS, SEG_EX_EPS, SEG_EX_EPS)
    return dict(partial=partial, dlogits=scatter(dz))


def seg_ref(inp):
    """float64 seg_loss forward and backward with GATHERS (tests/kernel_ref.py writes the interpolation as dense matrix
    products, whose zero entries would carry a NaN to pixels that never read the poisoned logit): partial [B, chunks, 4]
    = {sum bce, sum p t, sum p, sum t} over 8 output rows, and dlogits_lr [B, g, g] from the sums of those partials."""
    L, t, coef = inp["lr"].double(), inp["tgt"].double(), inp["coef"].double()
    B, g, S = L.shape[0], L.shape[-1], t.shape[-1]
    dev = L.device
    z, scatter, _ = seg_gather(L, S)
    e = torch.exp(-z.abs())
    p = torch.sigmoid(z)
    bce = z.clamp_min(0) - z * t + torch.log1p(e)
    chunks = (S + 7) // 8
    terms = torch.stack([bce, p * t, p, t], -1)
    pad = torch.zeros(B, chunks * 8 - S, S, 4, dtype=torch.float64, device=dev)
    partial = torch.cat([terms, pad], 1).view(B, chunks, 8, S, 4).sum((2, 3))
    sums = partial.sum(1)
    cb, cd = coef[:, 0, None, None], coef[:, 1, None, None]
    I, D = sums[:, 1, None, None], (sums[:, 2] + sums[:, 3] + SEG_EPS)[:, None, None]
    F = (2 * t * D - 2 * I) / (D * D)
    dz = cb * (p - t) + cd * (p * (1 - p)) * F
    dl = scatter(dz)
    return dict(partial=partial, dlogits=dl)


# ---- sums and copies ----------------------------------------------------------------------------------------------
SUM_DTYPES = [F32, BF16, F16]
COLSUM_SHAPES = [(1, 8), (512, 264), (1000, 136)]       # one row; two column blocks; two row chunks


def colsum_inputs(dtype, M, N, accumulate):
    g = torch.Generator(device="cpu").manual_seed(M + N)
    inp = dict(x=nonzero(torch.randn(M, N, generator=g).to(kr.TORCH_DT[dtype])))
    inp["prior"] = torch.randn(1, N, generator=g) * 5 if accumulate else None
    return inp


def colsum_sites(M, N):
    return sorted({("x", 0), ("x", M * N - 1), ("x", flat((M, N), (M - 1, N - 3)))})


def colsum_ref(inp):
    r = inp["x"].double().sum(0)
    return dict(out=r if inp["prior"] is None else r + inp["prior"].double()[0])


ADD_N = [5, 1027]                           # a tail only past one float4; 256 float4s and a 3-element tail


def add_inputs(n, with_b):
    g = torch.Generator(device="cpu").manual_seed(n)
    return dict(a=nonzero(torch.randn(n, generator=g)), b=nonzero(torch.randn(n, generator=g)) if with_b else None)


def add_sites(n, with_b):
    pos = sorted({0, n - 1, n - 3})
    return [(o, i) for o in (("a", "b") if with_b else ("a",)) for i in pos]


def add_ref(inp):
    return dict(out=inp["a"].double() if inp["b"] is None else inp["a"].double() + inp["b"].double())


VECMAT = [(5, 40), (300, 136)]              # rows, cols


def vecmat_inputs(rows, cols, accumulate):
    g = torch.Generator(device="cpu").manual_seed(rows + cols)
    inp = dict(v=nonzero(torch.randn(rows, generator=g)), W=nonzero(torch.randn(rows, cols, generator=g)))
    inp["prior"] = torch.randn(1, cols, generator=g) * 5 if accumulate else None
    return inp


def vecmat_sites(rows, cols):
    return [("v", 0), ("v", rows - 1), ("W", 0), ("W", rows * cols - 1), ("W", flat((rows, cols), (rows - 1, cols - 3)))]


def vecmat_ref(inp):
    r = (inp["v"].double()[:, None] * inp["W"].double()).sum(0)
    return dict(out=r if inp["prior"] is None else r + inp["prior"].double()[0])


BATCH_SUM = [(7, 257), (1, 255)]


def batch_sum_inputs(B, n, accumulate):
    g = torch.Generator(device="cpu").manual_seed(B + n)
    inp = dict(x=nonzero(torch.randn(B, n, generator=g)))
    inp["prior"] = torch.randn(1, n, generator=g) * 5 if accumulate else None
    return inp


def batch_sum_sites(B, n):
    return sorted({("x", 0), ("x", B * n - 1), ("x", flat((B, n), (B - 1, n - 3)))})


SPLIT3_C = [9, 144]                         # a partial last 8-chunk; the model's
SPLIT3_R = 5


def split3_inputs(C):
    g = torch.Generator(device="cpu").manual_seed(C)
    return dict(x=nonzero(torch.randn(SPLIT3_R, C, generator=g)))


def split3_sites(C):
    return [("x", 0), ("x", SPLIT3_R * C - 1), ("x", flat((SPLIT3_R, C), (SPLIT3_R - 1, C - 3)))]


def split3_ref(inp):
    """The value the three parts stand for: hi + lo = x (the a-side row is [hi | hi | lo], the b-side [hi | lo | hi])."""
    return dict(sum=inp["x"].double())


# ---- attention probabilities (sgl_op_attn_probs) -------------------------------------------------------------------
def probs_inputs(dtype, N, dh):
    """q, k of `attn_inputs` and the fp32 lse of their float64 scores, as a forward leaves them."""
    a = attn_inputs(dtype, N, dh)
    S = (a["q"].double() @ a["k"].double().transpose(-1, -2)) * dh ** -0.5
    return dict(q=a["q"], k=a["k"], lse=torch.logsumexp(S, -1).float())


def probs_sites(inp):
    """q and k at the positions of the attention table, lse at the first and the last query of head (1, 0).
    p = exp(S - lse): a score of -inf is probability 0, so q[i, c] = +-inf leaves the keys with the other sign of k[j, c]
    finite (and k[j, c] the queries likewise): each of the two values sits in the nearest column where the +inf scores are
    a majority.  lse = +inf makes every probability of the row 0, all excused wherever it sits: lse takes NaN and -inf."""
    shape = tuple(inp["q"].shape)
    N, dh = shape[2:]
    sites = []
    for o, other in (("q", "k"), ("k", "q")):
        vals = inp[other][ATTN_HEAD].double()
        for row, col in attn_positions(N, dh):
            at = {}
            for vn, v in VALUES:
                good = [c for c in range(dh) if vn == "nan" or int(((vals[:, c] * v) > 0).sum()) >= N // 2 + 1]
                at.setdefault(min(good, key=lambda c: (abs(c - col), c)), []).append(vn)
            sites += [(o, flat(shape, ATTN_HEAD + (row, c)), tuple(vns)) for c, vns in sorted(at.items())]
    return sites + [("lse", flat(shape[:3], ATTN_HEAD + (i,)), ("nan", "-inf")) for i in (0, N - 1)]


def probs_ref(inp):
    q, k, lse = inp["q"].double(), inp["k"].double(), inp["lse"].double()
    p = torch.exp((q @ k.transpose(-1, -2)) * q.shape[-1] ** -0.5 - lse[..., None])
    return dict(full=p, head_mean=p.mean(1))


# ---- fixed-order folds: reduce_partials, reduce_partials3, reduce_splits --------------------------------------------
RP_NBLK, RP_N = 9, 33                       # past the 8 row groups, one column past a 32-column group
RP3_NBLK, RP3_N = 25, 33                    # a column group that spans two outputs
RS_SHAPE, RS_SPLITS = (65, 132), 5


def fold_inputs(rows, cols, accumulate, prior_shape):
    g = torch.Generator(device="cpu").manual_seed(rows + cols)
    inp = dict(part=nonzero(torch.randn(rows, cols, generator=g)))
    inp["prior"] = torch.randn(*prior_shape, generator=g) * 5 if accumulate else None
    return inp


def fold_sites(rows, cols):
    return [("part", 0), ("part", rows * cols - 1), ("part", flat((rows, cols), (rows - 1, cols // 2 + 2)))]


def fold_ref(shape):
    def ref(inp):
        r = inp["part"].double().sum(0).view(*shape)
        return dict(out=r if inp["prior"] is None else r + inp["prior"].double().view(*shape))
    return ref


# ---- weight-shadow casts: cast_pad, cast_job -------------------------------------------------------------------------
CAST_PAD_SHAPES = [(1, 3), (65, 65)]        # R, C: one short row; one row and one column past 64


def cast_pad_inputs(R, C):
    g = torch.Generator(device="cpu").manual_seed(R + C)
    return dict(src=nonzero(torch.randn(R, C, generator=g) * 3))


def mat_sites(name, R, C):
    return sorted({(name, 0), (name, R * C - 1), (name, flat((R, C), (R - 1, max(C - 3, 0))))})


def cast_pad_ref(Rp, Cp):
    def ref(inp):
        R, C = inp["src"].shape
        out = torch.zeros(Rp, Cp, dtype=torch.float64, device=inp["src"].device)
        out[:R, :C] = inp["src"].double()
        return dict(dst=out)
    return ref


CAST_JOB = dict(R=65, C=33, lds=36, Rp=80, Cp=40, ldd=48, ldt=88, n=257, np=300)


def cast_job_inputs():
    g = torch.Generator(device="cpu").manual_seed(11)
    j = CAST_JOB
    return dict(mat=nonzero(torch.randn(j["R"], j["C"], generator=g) * 3), vec=nonzero(torch.randn(j["n"], generator=g)))


def cast_job_sites():
    j = CAST_JOB
    return mat_sites("mat", j["R"], j["C"]) + [("vec", 0), ("vec", j["n"] - 1)]


def cast_job_ref(inp):
    j = CAST_JOB
    d = cast_pad_ref(j["Rp"], j["Cp"])(dict(src=inp["mat"]))["dst"]
    v = torch.zeros(j["np"], dtype=torch.float64, device=d.device)
    v[:j["n"]] = inp["vec"].double()
    return dict(dst=d, dst_t=d.t(), vec=v)


# ---- im2col, col2im, pos_resize ------------------------------------------------------------------------------------------
IM2COL = [(2, 42, 28, 14, 0), (1, 42, 45, 14, 1)]       # B, H, W, P, channels_last: W != H; a remainder in W, NHWC storage


def im2col_inputs(B, H, W, P):
    g = torch.Generator(device="cpu").manual_seed(H + W)
    K = 3 * P * P
    L = (H // P) * (W // P)
    return dict(pix=nonzero(torch.randn(B, 3, H, W, generator=g)), cols=nonzero(torch.randn(B * L, K, generator=g)))


def im2col_sites(B, H, W, P):
    gh, gw = H // P, W // P
    sh = (B, 3, H, W)
    return [("pix", 0), ("pix", flat(sh, (B - 1, 2, gh * P - 1, gw * P - 1))), ("pix", flat(sh, (B - 1, 1, P, gw * P - 3)))]


def im2col_ref(P, Kp):
    def ref(inp):
        x = inp["pix"].double()
        B, _, H, W = x.shape
        gh, gw = H // P, W // P
        K = 3 * P * P
        u = torch.nn.functional.unfold(x[:, :, :gh * P, :gw * P], P, stride=P).transpose(1, 2).reshape(-1, K)
        out = torch.zeros(u.shape[0], Kp, dtype=torch.float64, device=x.device)
        out[:, :K] = u
        return dict(cols=out)
    return ref


def col2im_sites(B, H, W, P):
    K = 3 * P * P
    rows = B * (H // P) * (W // P)
    return mat_sites("cols", rows, K)


def col2im_ref(H, W, P):
    def ref(inp):
        c = inp["cols"].double()
        gh, gw = H // P, W // P
        B = c.shape[0] // (gh * gw)
        img = torch.nn.functional.fold(c.view(B, gh * gw, -1).transpose(1, 2), (gh * P, gw * P), P, stride=P)
        out = torch.zeros(B, 3, H, W, dtype=torch.float64, device=c.device)
        out[:, :, :gh * P, :gw * P] = img
        return dict(d_pixels=out)
    return ref


# g0, gh, gw: grids whose source positions never fall on a table entry, so no cubic weight is exactly zero and the
# reference (F.interpolate) and the kernel read the same sixteen taps with non-zero weights
POS_GRIDS = [(2, 3, 7), (14, 16, 27)]
POS_D = 40


def pos_inputs(g0, gh, gw, accumulate=True):
    g = torch.Generator(device="cpu").manual_seed(g0 * 100 + gh)
    return dict(table=nonzero(torch.randn(g0 * g0, POS_D, generator=g)), dout=nonzero(torch.randn(gh * gw, POS_D, generator=g)),
                prior=torch.randn(g0 * g0, POS_D, generator=g))


def pos_fwd_ref(g0, gh, gw):
    return lambda inp: dict(out=kr.pos_resize_ref(inp["table"], g0, gh, gw))


def pos_bwd_ref(g0, gh, gw):
    """prior + R^T dout by autograd through the float64 forward (a scatter: kernel_ref.pos_resize_bwd_ref multiplies by a
    dense matrix, whose zeros would carry a NaN to table entries that no poisoned output reads).  CPU only: the scatter's
    order is fixed there."""
    def ref(inp):
        t = torch.zeros(g0 * g0, POS_D, dtype=torch.float64, requires_grad=True)
        (gr,) = torch.autograd.grad(kr.pos_resize_ref(t, g0, gh, gw), t, inp["dout"].double().cpu())
        return dict(dtable=gr + inp["prior"].double().cpu())
    return ref


# ---- casts -------------------------------------------------------------------------------------------------------
CAST_DTYPES = [F32, BF16, F16]
CAST_N = 1027                               # 256 float4s and a 3-element tail


def cast_inputs():
    g = torch.Generator(device="cpu").manual_seed(3)
    return dict(src=nonzero(torch.randn(CAST_N, generator=g) * 3))


def cast_sites():
    return [("src", 0), ("src", CAST_N - 1), ("src", CAST_N - 3)]


def cast_ref(inp):
    return dict(dst=inp["src"].double())
