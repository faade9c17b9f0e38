"""CPU: the float64 reference of the attention-gradient kernels (tests/attn_grad_ref.py) against torch.autograd, an fp32
emulation against its bounds, the new symbols and their refusals (every one happens before anything is enqueued, so dummy
pointers do), ``heads.attention_relevance`` against the explicit matrix product, and the goldens' own consistency.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import abi_harness as ah
import attn_grad_ref as gr
import attn_probs_ref as ar

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "attngrad")
CASES = ["tiny_48", "tiny_208x176", "hostile_59x101"]
DUMMY = 0x7F0000001000          # never dereferenced
DTYPES = [ar.F32, ar.BF16, ar.BF16X3, ar.F16]
SHAPES = [(2, 4, 9, 16), (1, 2, 28, 72), (1, 3, 129, 64)]


def load_case(name):
    meta = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    grads = [torch.from_numpy(np.load(os.path.join(GOLDEN, f"{name}.l{i}.npz"))["attn_grad"])
             for i in range(int(meta["meta.layers"]))]
    return meta, grads


# ---------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_reference_is_autograds_gradient(shape):
    """dP of the reference = d/dP of sum(dO * (P V)) by torch.autograd in float64; PDP and RELEVANCE follow from it."""
    B, H, N, dh = shape
    q, k, v, dout, lse = gr.inputs(B, H, N, dh, ar.F32, seed=3)
    q64, k64, v64, g64 = q.double(), k.double(), v.double(), dout.double()
    P = torch.softmax((q64 @ k64.transpose(-1, -2)) * dh ** -0.5, -1).requires_grad_(True)
    (g64 * (P @ v64)).sum().backward()
    dP, _ = gr.grad_probs_ref(q, k, v, dout, lse, ar.F32, gr.DP)
    assert float((dP - P.grad).abs().max()) <= 1e-12 * float(P.grad.abs().max())
    lse64 = torch.logsumexp((q64 @ k64.transpose(-1, -2)) * dh ** -0.5, -1)
    pdp, _ = gr.grad_probs_ref(q, k, v, dout, lse64, ar.F32, gr.PDP)
    assert float((pdp - P.detach() * P.grad).abs().max()) <= 1e-12
    rel, _ = gr.grad_probs_ref(q, k, v, dout, lse64, ar.F32, gr.RELEVANCE)
    assert torch.equal(rel, torch.relu(pdp)) and float(rel.min()) == 0.0


@pytest.mark.parametrize("dtype", DTYPES, ids=[ar.DT_NAME[d] for d in DTYPES])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_fp32_emulation_stays_inside_the_bounds(shape, dtype):
    B, H, N, dh = shape
    q, k, v, dout, lse = gr.inputs(B, H, N, dh, dtype, seed=11 + N)
    for kind in gr.KINDS:
        ref, bound = gr.grad_probs_ref(q, k, v, dout, lse, dtype, kind)
        full = gr.emulate_fp32(q, k, v, dout, lse, kind, ar.FULL)
        w = gr.worst_ratio(full, ref, bound)
        m_ref, m_bound = gr.head_mean_ref(ref, bound)
        wm = gr.worst_ratio(gr.emulate_fp32(q, k, v, dout, lse, kind, ar.HEAD_MEAN), m_ref, m_bound)
        o_ref, o_bound = gr.head_mean_of_full(full)
        wo = gr.worst_ratio(gr.emulate_fp32(q, k, v, dout, lse, kind, ar.HEAD_MEAN), o_ref, o_bound)
        print(f"{ar.DT_NAME[dtype]} {shape} {gr.KIND_NAME[kind]}: full {w:.3f} mean {wm:.3f} mean-of-full {wo:.3f}")
        assert w <= 1.0 and wm <= 1.0 and wo <= 1.0
        assert float(bound.max()) <= 1e-3 * max(1.0, float(ref.abs().max()))          # and the bounds bind


def test_bounds_notice_a_wrong_kernel():
    """A dropped last column of V, a P taken without the lse shift, a plain fmax relu on a NaN: all outside."""
    B, H, N, dh = 1, 2, 28, 72
    q, k, v, dout, lse = gr.inputs(B, H, N, dh, ar.BF16, seed=5)
    ref, bound = gr.grad_probs_ref(q, k, v, dout, lse, ar.BF16, gr.DP)
    v_bad = v.clone()
    v_bad[..., -1] = 0
    assert gr.worst_ratio(gr.emulate_fp32(q, k, v_bad, dout, lse, gr.DP, ar.FULL), ref, bound) > 1.0
    ref, bound = gr.grad_probs_ref(q, k, v, dout, lse, ar.BF16, gr.PDP)
    assert gr.worst_ratio(gr.emulate_fp32(q, k, v, dout, lse * (1 + 2.0 ** -12), gr.PDP, ar.FULL), ref, bound) > 1.0
    x = torch.tensor([float("nan"), -1.0, 2.0])
    kept = gr.relu_keep_nan(x)
    assert bool(kept[0] != kept[0]) and kept[1] == 0 and kept[2] == 2


def test_pool_reference_is_autograds_gradient():
    B, H, N, dh = 2, 4, 9, 16
    g = torch.Generator().manual_seed(2)
    v = torch.randn(B, H, N, dh, generator=g)
    dout = torch.randn(B, H, dh, generator=g)
    p = torch.softmax(torch.randn(B, H, N, generator=g).double(), -1).requires_grad_(True)
    (dout.double() * torch.einsum("bhn,bhnd->bhd", p, v.double())).sum().backward()
    da, bound = gr.pool_ref(v, p.detach().float(), dout, gr.DP)
    assert float((da - p.grad).abs().max()) <= 1e-12
    got = torch.einsum("bhd,bhnd->bhn", dout, v)          # fp32
    assert gr.worst_ratio(got, da, bound) <= 1.0


# ---------------------------------------------------------------------------------------------------------------
# symbols and refusals
# ---------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = {"sgl_op_attn_grad_probs": 15, "sgl_op_pool_attn_grad_probs": 13, "sgl_backward_layer_pa": 17,
               "sgl_backward_begin_pa": 17}


def test_symbols_declared_exported_and_abi_unchanged(pkg, hiplib):
    declared = set(pkg.lib.declared_symbols())
    for name, nargs in NEW_SYMBOLS.items():
        assert name in declared, name
        assert len(getattr(hiplib, name).argtypes) == nargs, name
    assert hiplib.sgl_abi_version() == 3
    assert (pkg.lib.ATTN_GRAD_DP, pkg.lib.ATTN_GRAD_PDP, pkg.lib.ATTN_GRAD_RELEVANCE) == (0, 1, 2)
    with open(pkg.lib.HEADER_PATH) as f:
        text = f.read()
    assert "SGL_ATTN_GRAD_DP = 0, SGL_ATTN_GRAD_PDP = 1, SGL_ATTN_GRAD_RELEVANCE = 2" in text
    assert "sgl_attn_grad_req" in text
    assert C.sizeof(pkg.lib.SglAttnGradReq) == 24


OP_OK = dict(dtype=ar.BF16, q=DUMMY, k=DUMMY, v=DUMMY, dout=DUMMY, lse=DUMMY, out=DUMMY, B=2, H=4, N=9, dh=72, DP=80,
             kind=gr.RELEVANCE, mode=ar.FULL)
OP_REFUSALS = [
    ("q NULL", dict(q=None), ah.ERR_NULL), ("k NULL", dict(k=None), ah.ERR_NULL), ("v NULL", dict(v=None), ah.ERR_NULL),
    ("dout NULL", dict(dout=None), ah.ERR_NULL), ("lse NULL", dict(lse=None), ah.ERR_NULL),
    ("out NULL", dict(out=None), ah.ERR_NULL),
    ("B = 0", dict(B=0), ah.ERR_BAD_SHAPE), ("H = 0", dict(H=0), ah.ERR_BAD_SHAPE), ("N = 0", dict(N=0), ah.ERR_BAD_SHAPE),
    ("N < 0", dict(N=-3), ah.ERR_BAD_SHAPE), ("head_dim = 0", dict(dh=0), ah.ERR_BAD_SHAPE),
    ("head_dim > head_dim_pad", dict(dh=88, DP=80), ah.ERR_BAD_SHAPE),
    ("head_dim_pad not round_up(head_dim, 16)", dict(DP=96), ah.ERR_BAD_SHAPE),
    ("head_dim % 8", dict(dh=20, DP=32), ah.ERR_BAD_SHAPE),
    ("head_dim_pad > 96", dict(dh=104, DP=112), ah.ERR_BAD_SHAPE),
    ("fp16: head_dim_pad not round_up", dict(dtype=ar.F16, DP=96), ah.ERR_BAD_SHAPE),
    ("bf16x3: head_dim > 96", dict(dtype=ar.BF16X3, dh=104, DP=112), ah.ERR_BAD_SHAPE),
    ("fp32: head_dim > 128", dict(dtype=ar.F32, dh=136, DP=144), ah.ERR_BAD_SHAPE),
    ("bf16: dout rows past 2^31 bytes", dict(H=64, N=1 << 18, dh=64, DP=64), ah.ERR_BAD_SHAPE),
    ("dtype 4", dict(dtype=4), ah.ERR_UNSUPPORTED), ("dtype mxfp8", dict(dtype=5), ah.ERR_UNSUPPORTED),
    ("dtype -1", dict(dtype=-1), ah.ERR_UNSUPPORTED),
    ("mode 2", dict(mode=2), ah.ERR_UNSUPPORTED), ("mode -1", dict(mode=-1), ah.ERR_UNSUPPORTED),
    ("kind 3", dict(kind=3), ah.ERR_UNSUPPORTED), ("kind -1", dict(kind=-1), ah.ERR_UNSUPPORTED),
    ("misaligned q", dict(q=DUMMY + 8), ah.ERR_UNSUPPORTED), ("misaligned k", dict(k=DUMMY + 2), ah.ERR_UNSUPPORTED),
    ("misaligned v", dict(v=DUMMY + 4), ah.ERR_UNSUPPORTED), ("misaligned dout", dict(dout=DUMMY + 8), ah.ERR_UNSUPPORTED),
    # the order of sgl_op_attn_probs: NULL, dimensions, dtype, mode, kind, shape contract
    ("NULL before shape", dict(q=None, B=0, dtype=9), ah.ERR_NULL),
    ("dimension before dtype", dict(B=0, dtype=9, kind=9), ah.ERR_BAD_SHAPE),
    ("dtype before contract", dict(dtype=9, DP=96), ah.ERR_UNSUPPORTED),
    ("kind before contract", dict(kind=9, DP=96), ah.ERR_UNSUPPORTED),
]


def call_op(lib, a):
    return lib.sgl_op_attn_grad_probs(a["dtype"], a["q"], a["k"], a["v"], a["dout"], a["lse"], a["out"], a["B"], a["H"],
                                      a["N"], a["dh"], a["DP"], a["kind"], a["mode"], None)


@pytest.mark.parametrize("what,change,status", OP_REFUSALS, ids=[r[0] for r in OP_REFUSALS])
def test_op_refusals(hiplib, what, change, status):
    st = call_op(hiplib, {**OP_OK, **change})
    assert st == status, f"{what}: status {st}, expected {status}"


POOL_OK = dict(dtype=ar.BF16, V=DUMMY, probs=DUMMY, dout=DUMMY, out=DUMMY, B=2, H=4, N=9, dh=72, DP=80, kind=gr.RELEVANCE,
               mode=ar.FULL)
POOL_REFUSALS = [
    ("V NULL", dict(V=None), ah.ERR_NULL), ("probs NULL", dict(probs=None), ah.ERR_NULL),
    ("dout NULL", dict(dout=None), ah.ERR_NULL), ("out NULL", dict(out=None), ah.ERR_NULL),
    ("B = 0", dict(B=0), ah.ERR_BAD_SHAPE), ("N = 0", dict(N=0), ah.ERR_BAD_SHAPE), ("H < 0", dict(H=-1), ah.ERR_BAD_SHAPE),
    ("head_dim % 8", dict(dh=20, DP=32), ah.ERR_BAD_SHAPE), ("head_dim > head_dim_pad", dict(dh=88), ah.ERR_BAD_SHAPE),
    ("head_dim_pad % 8", dict(DP=84), ah.ERR_BAD_SHAPE),
    ("dtype bf16x3", dict(dtype=ar.BF16X3), ah.ERR_UNSUPPORTED), ("dtype 7", dict(dtype=7), ah.ERR_UNSUPPORTED),
    ("misaligned V", dict(V=DUMMY + 8), ah.ERR_UNSUPPORTED),
    ("mode 2", dict(mode=2), ah.ERR_UNSUPPORTED), ("kind 3", dict(kind=3), ah.ERR_UNSUPPORTED),
    ("kind -1", dict(kind=-1), ah.ERR_UNSUPPORTED),
]


def call_pool(lib, a):
    return lib.sgl_op_pool_attn_grad_probs(a["dtype"], a["V"], a["probs"], a["dout"], a["out"], a["B"], a["H"], a["N"],
                                           a["dh"], a["DP"], a["kind"], a["mode"], None)


@pytest.mark.parametrize("what,change,status", POOL_REFUSALS, ids=[r[0] for r in POOL_REFUSALS])
def test_pool_op_refusals(hiplib, what, change, status):
    st = call_pool(hiplib, {**POOL_OK, **change})
    assert st == status, f"{what}: status {st}, expected {status}"


class PaCtx:
    """A context and dummy arenas for the two _pa entry points: every refusal of a request precedes any device work."""

    def __init__(self, pkg, lib, cfg_name="hostile", mode="bf16", recompute=0, use_head=1, B=2, H=42, W=70):
        self.pkg, self.lib = pkg, lib
        self.cfg = ah.make_config(pkg, cfg_name, use_head)
        self.ctx = lib.sgl_create_ex(C.byref(ah.sgl_config(pkg, self.cfg, mode, use_head)), recompute)
        assert self.ctx
        self.B, self.H, self.W = B, H, W
        self.L, self.heads = self.cfg.num_hidden_layers, self.cfg.num_attention_heads
        self.N = (H // self.cfg.patch_size) * (W // self.cfg.patch_size)
        a, b, c = C.c_size_t(), C.c_size_t(), C.c_size_t()
        if mode == "mxfp8":
            b.value = c.value = 1 << 20
        else:
            assert lib.sgl_query_sizes(self.ctx, B, H, W, 1, C.byref(a), C.byref(b), C.byref(c)) == ah.OK
        self.saved_bytes, self.ws_bytes = b.value, c.value
        self.w, self._wl = ah.weights_struct(pkg, self.cfg, lambda n: DUMMY)
        self.g = pkg.lib.SglGrads()
        self._gl = (pkg.lib.SglLayerPtrs * max(self.L, 1))()
        self.g.layers = C.cast(self._gl, C.POINTER(pkg.lib.SglLayerPtrs))

    def req(self, out=DUMMY, out_bytes=1 << 40, kind=gr.RELEVANCE, mode=ar.HEAD_MEAN):
        return self.pkg.lib.SglAttnGradReq(out, out_bytes, kind, mode)

    def layer(self, req, layer=0, saved_bytes=None):
        sb = self.saved_bytes if saved_bytes is None else saved_bytes
        return self.lib.sgl_backward_layer_pa(self.ctx, C.byref(self.w), DUMMY, C.byref(self.g), layer, self.B, self.H,
                                              self.W, DUMMY, None, 1, DUMMY, sb, DUMMY, self.ws_bytes, None,
                                              C.byref(req) if req is not None else None)

    def begin(self, req, d_pooled=DUMMY, saved_bytes=None):
        sb = self.saved_bytes if saved_bytes is None else saved_bytes
        return self.lib.sgl_backward_begin_pa(self.ctx, C.byref(self.w), DUMMY, C.byref(self.g), self.B, self.H, self.W,
                                              DUMMY, None, d_pooled, None, DUMMY, sb, DUMMY, self.ws_bytes, None,
                                              C.byref(req) if req is not None else None)

    def close(self):
        self.lib.sgl_destroy(self.ctx)


@pytest.fixture()
def pa(pkg, hiplib):
    c = PaCtx(pkg, hiplib)
    yield c
    c.close()


def test_pa_request_refusals(pa):
    B, Hh, N = pa.B, pa.heads, pa.N
    for call, rows in ((pa.layer, N), (pa.begin, 1)):
        assert call(pa.req(out=None)) == ah.ERR_NULL
        assert call(pa.req(kind=3)) == ah.ERR_UNSUPPORTED and call(pa.req(kind=-1)) == ah.ERR_UNSUPPORTED
        assert call(pa.req(mode=2)) == ah.ERR_UNSUPPORTED and call(pa.req(mode=-1)) == ah.ERR_UNSUPPORTED
        assert call(pa.req(out_bytes=B * rows * N * 4 - 1)) == ah.ERR_WORKSPACE
        assert call(pa.req(mode=ar.FULL, out_bytes=B * Hh * rows * N * 4 - 1)) == ah.ERR_WORKSPACE
        # the plain call's checks come first, the request's NULL before its kind, its kind before its size
        assert call(pa.req(out=None), saved_bytes=0) == ah.ERR_WORKSPACE
        assert call(pa.req(out=None, kind=9, out_bytes=0)) == ah.ERR_NULL
        assert call(pa.req(kind=9, out_bytes=0)) == ah.ERR_UNSUPPORTED
    assert pa.layer(pa.req(), layer=pa.L) == ah.ERR_BAD_SHAPE
    assert pa.begin(pa.req(), d_pooled=None) == ah.ERR_UNSUPPORTED          # no d_pooled: the head is not differentiated


def test_pa_context_refusals(pkg, hiplib):
    for kw in (dict(recompute=1), dict(mode="mxfp8")):
        c = PaCtx(pkg, hiplib, **kw)
        try:
            assert c.layer(c.req()) == ah.ERR_UNSUPPORTED, kw
            assert c.begin(c.req()) == ah.ERR_UNSUPPORTED, kw
        finally:
            c.close()
    c = PaCtx(pkg, hiplib, use_head=0)
    try:
        assert c.begin(c.req()) == ah.ERR_UNSUPPORTED
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------------------------
# heads.attention_relevance
# ---------------------------------------------------------------------------------------------------------------
def relevance_bound(maps64, pooling64=None):
    """fp32 evaluation of prod (I + A_l) [and the row through it] on non-negative maps: every entry is a sum of products
    of at most L factors over at most N-term sums, all non-negative, so each of the L (+ 1) bmm steps and additions
    multiplies the relative error by at most (1 + u)^(N + 1): relative (L + 2)(N + 2) u overall (first order, doubled for
    the second-order terms), plus the fp32 rounding of the inputs, 2 u per factor."""
    L, N = len(maps64), maps64[0].shape[-1]
    return 2 * ((L + 2) * (N + 2) + 2 * (L + 1)) * ar.EPS32


@pytest.mark.parametrize("B,N,L", [(2, 9, 3), (1, 37, 5)])
def test_attention_relevance_is_the_matrix_product(pkg, B, N, L):
    g = torch.Generator().manual_seed(N)
    maps = [torch.rand(B, N, N, generator=g, dtype=torch.float64) / N for _ in range(L)]
    pool = torch.rand(B, N, generator=g, dtype=torch.float64)
    eye = torch.eye(N, dtype=torch.float64)
    R = eye.expand(B, N, N)
    for A in maps:                      # last block leftmost
        R = (eye + A) @ R
    got = pkg.heads.attention_relevance([m.float() for m in maps])
    assert got.dtype == torch.float32 and got.shape == (B, N, N)
    tol = relevance_bound(maps)
    assert float(((got.double() - R).abs() / R.clamp_min(1e-300)).max()) <= tol
    row = pkg.heads.attention_relevance([m.float() for m in maps], pooling=pool.float())
    want = (pool.unsqueeze(1) @ R).squeeze(1)
    assert row.shape == (B, N) and float(((row.double() - want).abs() / want).max()) <= tol
    # the row-vector recurrence model.attention_relevance runs, in backward order: r <- r + r A_l from r = pool
    r = pool.clone()
    for A in reversed(maps):
        r = r + (r.unsqueeze(1) @ A).squeeze(1)
    assert float(((r - want).abs() / want).max()) <= 1e-13
    # per-head inputs are averaged first
    per_head = [torch.stack([m.float() * 0.5, m.float() * 1.5], 1) for m in maps]
    assert float(((pkg.heads.attention_relevance(per_head).double() - R).abs() / R.clamp_min(1e-300)).max()) <= tol
    with pytest.raises(ValueError):
        pkg.heads.attention_relevance([])


# ---------------------------------------------------------------------------------------------------------------
# goldens
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_goldens_are_consistent(pkg, name):
    """Shapes, HF's own autocast yardsticks, and the stored relevance = heads.attention_relevance of the stored maps'
    relu(A * grad A) head means read through the pooling row (the attention goldens hold A)."""
    from test_attn_maps_host import load_case as load_attn
    meta, grads = load_case(name)
    ameta, att = load_attn(name)
    cfg = pkg.get_config(str(meta["meta.config"]))
    B, H, W = int(meta["meta.batch"]), int(meta["meta.res_h"]), int(meta["meta.res_w"])
    N = (H // cfg.patch_size) * (W // cfg.patch_size)
    assert len(grads) == cfg.num_hidden_layers == len(att)
    for g, a in zip(grads, att):
        assert g.shape == (B, cfg.num_attention_heads, N, N) == a.shape and bool(torch.isfinite(g).all())
    for tag in ("bf16ac.", "fp16ac."):
        y = meta[tag + "attn_grad.l2rel"]
        assert y.shape == (len(grads),) and bool((y > 0).all()) and bool((y < 0.2).all())
    assert meta["pooling_grad"].shape == (B, cfg.num_attention_heads, N)
    assert meta["relevance"].shape == (B, N) and meta["relevance"].dtype == np.float64
    maps = [torch.relu(a.double() * g.double()).mean(1) for a, g in zip(att, grads)]
    pool = torch.relu(torch.from_numpy(ameta["pooling"]).double() * torch.from_numpy(meta["pooling_grad"]).double()).mean(1)
    r = pool.clone()
    for A in reversed(maps):
        r = r + (r.unsqueeze(1) @ A).squeeze(1)
    ref = torch.from_numpy(meta["relevance"])
    # the stored maps are fp32 roundings of what the float64 relevance was composed from
    assert float((r - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
    assert float(meta["restatement.pooled_err"]) <= 1e-5 and float(meta["restatement.dlast_err"]) <= 1e-5
