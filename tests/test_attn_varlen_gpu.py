"""The ragged (varlen) kernels through the C ABI: sgl_op_attn_fwd_varlen, sgl_op_pool_attn_fwd_varlen, sgl_op_seg_offsets.

The strongest statement available needs no tolerance: segment s of a packed batch must get, bit for bit, what the fixed
kernel gives that segment alone (B = 1, N = n_s).  The segment lengths sit at the edges of the 32-row wave tile, the
64-key tile and the 128-row query block and make every segment start unaligned; H = 3 and 9 make S * H no multiple of
the 8 XCDs.  One case per route is also held element-wise to the float64 reference with the bounds of kernel_ref,
unchanged.  Every output sits between sentinel rows."""
import ctypes as C

import numpy as np
import pytest
import torch

import kernel_ref as kr
from attn_util import DEV, Guarded, P, ok, rup, stream, tdt_of
from kernel_ref import BF16, BF16X3, F16, F32
from op_runners import run_pool_attn_fwd

pytestmark = pytest.mark.gpu

LENS = [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257, 1]
S = len(LENS)
CU = [0] + [int(v) for v in np.cumsum(LENS)]
T = CU[-1]
MAX_N = max(LENS)
assert T == 931
HEADS = [3, 9]
DIMS = [(72, 80), (64, 64), (16, 16)]
DTYPES = [BF16, F16, F32, BF16X3]
IDS = {BF16: "bf16", F16: "f16", F32: "f32", BF16X3: "bf16x3"}


def bits(t):
    """The tensor's bit patterns, so that equal means bit-identical (NaN included)."""
    t = t.contiguous()
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


def seg_table(lib, lens):
    """The device table of sgl_op_seg_offsets, between sentinels."""
    g = Guarded(1, len(lens) + 1, len(lens) + 1, torch.int32, prior=-7)
    ok(lib.sgl_op_seg_offsets((C.c_int * len(lens))(*lens), len(lens), g.ptr, stream()))
    torch.cuda.synchronize()
    return g


_TABLE = {}


def cu_dev(lib):
    if "cu" not in _TABLE:
        _TABLE["cu"] = seg_table(lib, LENS)
    return _TABLE["cu"]


def packed(x, DP):
    """[1, H, T, dh] -> head-major [H, T, DP] with zero pad columns, on the device."""
    _, H, n, dh = x.shape
    out = torch.zeros(H, n, DP, dtype=x.dtype, device=DEV)
    out[..., :dh] = x[0].to(DEV)
    return out


_INPUTS = {}


def attn_case(dtype, H, dh, DP):
    """q | k | v of one packed batch, [3, H, T, DP] (computed once per case, never modified)."""
    key = (dtype, H, dh)
    if key not in _INPUTS:
        q, k, v, _ = kr.attn_inputs("gauss", 1, H, T, dh, tdt_of(dtype), seed=H + dh)
        _INPUTS[key] = torch.stack([packed(t, DP) for t in (q, k, v)])
    return _INPUTS[key]


def run_varlen(lib, dtype, qkv, H, dh, DP, max_n=MAX_N, written=True):
    """sgl_op_attn_fwd_varlen on [3, H, T, DP]: out [T, H * dh] and lse [H, T], guard bands checked."""
    out = Guarded(T, H * dh, H * dh, tdt_of(dtype))
    lse = Guarded(1, H * T, H * T, torch.float32)
    ok(lib.sgl_op_attn_fwd_varlen(dtype, P(qkv[0]), P(qkv[1]), P(qkv[2]), out.ptr, lse.ptr, cu_dev(lib).ptr, S, T, max_n, H,
                                  dh, DP, stream()))
    torch.cuda.synchronize()
    out.check("varlen out", written)
    lse.check("varlen lse", written)
    cu_dev(lib).check("cu", written=False)
    return out.got().clone(), lse.got().view(H, T).clone()


def run_fixed(lib, dtype, qkv, s, H, dh, DP):
    """sgl_op_attn_fwd(B = 1, N = n_s, ld_qkv = 0) on the contiguous copy of segment s: out [n, H * dh], lse [H, n]."""
    a, b = CU[s], CU[s + 1]
    n = b - a
    seg = qkv[:, :, a:b].contiguous()
    out = Guarded(n, H * dh, H * dh, tdt_of(dtype))
    lse = Guarded(1, H * n, H * n, torch.float32)
    ok(lib.sgl_op_attn_fwd(dtype, P(seg[0]), P(seg[1]), P(seg[2]), out.ptr, lse.ptr, 1, H, n, dh, DP, 0, stream()))
    torch.cuda.synchronize()
    out.check("fixed out")
    lse.check("fixed lse")
    return out.got(), lse.got().view(H, n)


@pytest.mark.parametrize("dh,DP", DIMS, ids=[f"dh{d}" for d, _ in DIMS])
@pytest.mark.parametrize("H", HEADS)
@pytest.mark.parametrize("dtype", DTYPES, ids=[IDS[d] for d in DTYPES])
def test_segments_equal_the_fixed_kernel_bitwise(hiplib, dtype, H, dh, DP):
    qkv = attn_case(dtype, H, dh, DP)
    out, lse = run_varlen(hiplib, dtype, qkv, H, dh, DP)
    for s in range(S):
        o, l = run_fixed(hiplib, dtype, qkv, s, H, dh, DP)
        a, b = CU[s], CU[s + 1]
        assert torch.equal(bits(out[a:b]), bits(o)), f"segment {s} (n = {b - a}): out differs from the fixed kernel"
        assert torch.equal(bits(lse[:, a:b]), bits(l)), f"segment {s} (n = {b - a}): lse differs from the fixed kernel"


@pytest.mark.parametrize("dtype", DTYPES, ids=[IDS[d] for d in DTYPES])
def test_segments_within_the_float64_bound(hiplib, dtype):
    H, dh, DP = 3, 72, 80
    qkv = attn_case(dtype, H, dh, DP)
    out, lse = run_varlen(hiplib, dtype, qkv, H, dh, DP)
    u = kr.UNIT[tdt_of(dtype)]
    for s in range(S):
        a, b = CU[s], CU[s + 1]
        q, k, v = (qkv[j, :, a:b, :dh] for j in range(3))
        r = kr.attn_ref(q, k, v)
        bO, bl = kr.attn_fwd_bound(r, u, dtype in (F32, BF16X3))
        O = out[a:b].view(b - a, H, dh).permute(1, 0, 2)
        kr.assert_within(O, r["O"], bO, f"varlen {IDS[dtype]} segment {s} O")
        kr.assert_within(lse[:, a:b], r["lse"], bl, f"varlen {IDS[dtype]} segment {s} lse")


@pytest.mark.parametrize("s", [0, 6, S - 1], ids=["first", "middle", "last"])
@pytest.mark.parametrize("dtype", DTYPES, ids=[IDS[d] for d in DTYPES])
def test_a_segment_never_sees_its_neighbours(hiplib, dtype, s):
    H, dh, DP = 3, 72, 80
    qkv = attn_case(dtype, H, dh, DP)
    out, lse = run_varlen(hiplib, dtype, qkv, H, dh, DP)
    a, b = CU[s], CU[s + 1]
    poisoned = torch.full_like(qkv, float("nan"))
    poisoned[:, :, a:b] = qkv[:, :, a:b]
    pout, plse = run_varlen(hiplib, dtype, poisoned, H, dh, DP, written=False)
    assert torch.equal(bits(pout[a:b]), bits(out[a:b])), f"segment {s}: out changed when the other segments became NaN"
    assert torch.equal(bits(plse[:, a:b]), bits(lse[:, a:b])), f"segment {s}: lse changed when the others became NaN"


@pytest.mark.parametrize("dtype", DTYPES, ids=[IDS[d] for d in DTYPES])
def test_two_calls_and_a_larger_max_n_give_the_same_bits(hiplib, dtype):
    H, dh, DP = 9, 72, 80
    qkv = attn_case(dtype, H, dh, DP)
    out, lse = run_varlen(hiplib, dtype, qkv, H, dh, DP)
    for max_n, what in ((MAX_N, "a second call"), (384, "max_n = 384")):
        o, l = run_varlen(hiplib, dtype, qkv, H, dh, DP, max_n=max_n)
        assert torch.equal(bits(o), bits(out)) and torch.equal(bits(l), bits(lse)), f"{what} changed the result"


# ---- the pooling head's kernel -----------------------------------------------------------------------------------
POOL_DTYPES = [BF16, F16, F32]
_POOL = {}


def pool_case(dtype, H, dh, DP):
    key = (dtype, H, dh)
    if key not in _POOL:
        q, K, V, _ = kr.pool_inputs("gauss", 1, H, T, dh, DP, tdt_of(dtype), seed=H + dh)
        _POOL[key] = (q.to(DEV), K[0].to(DEV).contiguous(), V[0].to(DEV).contiguous())
    return _POOL[key]


def run_pool_varlen(lib, dtype, q, K, V, H, dh, DP, max_n=MAX_N, written=True):
    out = Guarded(S, H * dh, H * dh, tdt_of(dtype))
    probs = Guarded(1, H * T, H * T, torch.float32)
    ok(lib.sgl_op_pool_attn_fwd_varlen(dtype, P(q), P(K), P(V), out.ptr, probs.ptr, cu_dev(lib).ptr, S, T, max_n, H, dh, DP,
                                       stream()))
    torch.cuda.synchronize()
    out.check("pool varlen out", written)
    probs.check("pool varlen probs", written)
    return out.got().clone(), probs.got().view(H, T).clone()


@pytest.mark.parametrize("dh,DP", DIMS, ids=[f"dh{d}" for d, _ in DIMS])
@pytest.mark.parametrize("H", HEADS)
@pytest.mark.parametrize("dtype", POOL_DTYPES, ids=[IDS[d] for d in POOL_DTYPES])
def test_pool_segments_equal_the_fixed_kernel_bitwise(hiplib, dtype, H, dh, DP):
    q, K, V = pool_case(dtype, H, dh, DP)
    out, probs = run_pool_varlen(hiplib, dtype, q, K, V, H, dh, DP)
    for s in range(S):
        a, b = CU[s], CU[s + 1]
        Ks, Vs = K[:, a:b].contiguous(), V[:, a:b].contiguous()
        o, p = run_pool_attn_fwd(hiplib, dtype, q, Ks, Vs, 1, H, b - a, dh, DP)
        o.check("pool fixed out")
        p.check("pool fixed probs")
        assert torch.equal(bits(out[s]), bits(o.got()[0])), f"segment {s}: pooled out differs from the fixed kernel"
        assert torch.equal(bits(probs[:, a:b]), bits(p.got())), f"segment {s}: probs differ from the fixed kernel"
    o2, p2 = run_pool_varlen(hiplib, dtype, q, K, V, H, dh, DP)
    o3, p3 = run_pool_varlen(hiplib, dtype, q, K, V, H, dh, DP, max_n=384)
    for o, p, what in ((o2, p2, "a second call"), (o3, p3, "max_n = 384")):
        assert torch.equal(bits(o), bits(out)) and torch.equal(bits(p), bits(probs)), f"{what} changed the result"


@pytest.mark.parametrize("dtype", POOL_DTYPES, ids=[IDS[d] for d in POOL_DTYPES])
def test_pool_segments_within_the_float64_bound(hiplib, dtype):
    H, dh, DP = 3, 72, 80
    q, K, V = pool_case(dtype, H, dh, DP)
    out, probs = run_pool_varlen(hiplib, dtype, q, K, V, H, dh, DP)
    for s in range(S):
        a, b = CU[s], CU[s + 1]
        (Pr, bP), (o, bo) = kr.pool_attn_fwd_ref(q, K[None, :, a:b], V[None, :, a:b], H, dh, tdt_of(dtype))
        kr.assert_within(probs[None, :, a:b], Pr, bP, f"pool varlen {IDS[dtype]} segment {s} probs")
        kr.assert_within(out[s:s + 1], o, bo, f"pool varlen {IDS[dtype]} segment {s} out")


@pytest.mark.parametrize("s", [0, 6, S - 1], ids=["first", "middle", "last"])
def test_pool_segment_never_sees_its_neighbours(hiplib, s):
    dtype, H, dh, DP = BF16, 3, 72, 80
    q, K, V = pool_case(dtype, H, dh, DP)
    out, probs = run_pool_varlen(hiplib, dtype, q, K, V, H, dh, DP)
    a, b = CU[s], CU[s + 1]
    Kp, Vp = torch.full_like(K, float("nan")), torch.full_like(V, float("nan"))
    Kp[:, a:b], Vp[:, a:b] = K[:, a:b], V[:, a:b]
    pout, pprobs = run_pool_varlen(hiplib, dtype, q, Kp, Vp, H, dh, DP, written=False)
    assert torch.equal(bits(pout[s]), bits(out[s])) and torch.equal(bits(pprobs[:, a:b]), bits(probs[:, a:b])), \
        f"segment {s}: the pooled result changed when the other segments became NaN"


# ---- the table writer --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 64, 65, 1000])
def test_seg_offsets_equal_numpy_cumsum(hiplib, n):
    lens = list(np.random.default_rng(n).integers(0, 1500, size=n))
    g = seg_table(hiplib, [int(v) for v in lens])
    g.check("cu", written=False)
    want = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    assert np.array_equal(g.got().cpu().numpy()[0], want)
