"""CPU (no GPU): the attention-map feature's refusals, its plain-torch rollout and its fixtures.

* every documented refusal of ``sgl_op_attn_probs`` and ``sgl_attention_probs`` with its status code.  Each call is invalid
  in exactly one argument and returns before the first HIP call; device pointers are dummy integers nobody dereferences
  (the pattern of tests/test_abi_contract_host.py: were a check missing, the call would reach the HIP runtime and come back
  as SGL_ERR_HIP on a machine without a device).
* ``heads.attention_rollout`` against a float64 loop on the golden HF maps.
* the goldens of tests/gen_golden_attn.py load and HF's rows sum to 1.
* the errors of the Python surface that are raised before any device work.
"""
import ctypes as C
import glob
import os

import numpy as np
import pytest
import torch

import abi_harness as ah
import attn_probs_ref as ar

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "attn")
CASES = ["tiny_48", "tiny_37x45", "tiny_208x176", "hostile_59x101"]
DUMMY = 0x7F0000001000          # never dereferenced


def load_case(name):
    meta = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    att = [torch.from_numpy(np.load(os.path.join(GOLDEN, f"{name}.l{i}.npz"))["attentions"])
           for i in range(int(meta["meta.layers"]))]
    return meta, att


# ---------------------------------------------------------------------------------------------------------------
# sgl_op_attn_probs
# ---------------------------------------------------------------------------------------------------------------
OP_OK = dict(dtype=ar.BF16, q=DUMMY, k=DUMMY, lse=DUMMY, out=DUMMY, B=2, H=4, N=9, dh=72, DP=80, mode=ar.FULL)
OP_REFUSALS = [
    ("q NULL", dict(q=None), ah.ERR_NULL), ("k NULL", dict(k=None), ah.ERR_NULL),
    ("lse NULL", dict(lse=None), ah.ERR_NULL), ("out NULL", dict(out=None), ah.ERR_NULL),
    ("B = 0", dict(B=0), ah.ERR_BAD_SHAPE), ("H = 0", dict(H=0), ah.ERR_BAD_SHAPE), ("N = 0", dict(N=0), ah.ERR_BAD_SHAPE),
    ("N < 0", dict(N=-3), ah.ERR_BAD_SHAPE), ("head_dim = 0", dict(dh=0), ah.ERR_BAD_SHAPE),
    ("head_dim > head_dim_pad", dict(dh=88, DP=80), ah.ERR_BAD_SHAPE),
    ("head_dim_pad not round_up(head_dim, 16)", dict(DP=96), ah.ERR_BAD_SHAPE),
    ("head_dim % 8", dict(dh=20, DP=32), ah.ERR_BAD_SHAPE),
    ("head_dim_pad > 96", dict(dh=104, DP=112), ah.ERR_BAD_SHAPE),
    ("fp16: head_dim_pad not round_up", dict(dtype=ar.F16, DP=96), ah.ERR_BAD_SHAPE),
    ("bf16x3: head_dim > 96", dict(dtype=ar.BF16X3, dh=104, DP=112), ah.ERR_BAD_SHAPE),
    ("fp32: head_dim > 128", dict(dtype=ar.F32, dh=136, DP=144), ah.ERR_BAD_SHAPE),
    ("dtype 4", dict(dtype=4), ah.ERR_UNSUPPORTED), ("dtype mxfp8", dict(dtype=5), ah.ERR_UNSUPPORTED),
    ("dtype -1", dict(dtype=-1), ah.ERR_UNSUPPORTED),
    ("mode 2", dict(mode=2), ah.ERR_UNSUPPORTED), ("mode -1", dict(mode=-1), ah.ERR_UNSUPPORTED),
    ("misaligned q", dict(q=DUMMY + 8), ah.ERR_UNSUPPORTED), ("misaligned k", dict(k=DUMMY + 2), ah.ERR_UNSUPPORTED),
]


@pytest.mark.parametrize("what,change,status", OP_REFUSALS, ids=[r[0] for r in OP_REFUSALS])
def test_op_refusals(hiplib, what, change, status):
    a = {**OP_OK, **change}
    st = hiplib.sgl_op_attn_probs(a["dtype"], a["q"], a["k"], a["lse"], a["out"], a["B"], a["H"], a["N"], a["dh"], a["DP"],
                                  a["mode"], None)
    assert st == status, f"{what}: status {st}, expected {status}"


def test_symbols_declared_with_argtypes(pkg, hiplib):
    assert {"sgl_op_attn_probs", "sgl_attention_probs"} <= set(pkg.lib.declared_symbols())
    assert len(hiplib.sgl_op_attn_probs.argtypes) == 12 and len(hiplib.sgl_attention_probs.argtypes) == 11
    assert hiplib.sgl_abi_version() == 3


# ---------------------------------------------------------------------------------------------------------------
# sgl_attention_probs
# ---------------------------------------------------------------------------------------------------------------
class Ctx:
    def __init__(self, pkg, lib, cfg_name="hostile", mode="bf16", recompute=0, use_head=1, B=2, H=42, W=70):
        self.lib = lib
        self.cfg = ah.make_config(pkg, cfg_name, use_head)
        self.ctx = lib.sgl_create_ex(C.byref(ah.sgl_config(pkg, self.cfg, mode, use_head)), recompute)
        assert self.ctx
        self.B, self.H, self.W = B, H, W
        self.L, self.heads = self.cfg.num_hidden_layers, self.cfg.num_attention_heads
        self.N = (H // self.cfg.patch_size) * (W // self.cfg.patch_size)
        a, b, c = C.c_size_t(), C.c_size_t(), C.c_size_t()
        if mode == "mxfp8":          # no training sizes exist: any arena size will do, the mode is refused first
            b.value = 1 << 20
        else:
            assert lib.sgl_query_sizes(self.ctx, B, H, W, 1, C.byref(a), C.byref(b), C.byref(c)) == ah.OK
        self.saved_bytes = b.value

    def call(self, **change):
        a = dict(ctx=self.ctx, B=self.B, H=self.H, W=self.W, saved=DUMMY, saved_bytes=self.saved_bytes, layer=0,
                 mode=ar.FULL, out=DUMMY, out_bytes=1 << 40)
        a.update(change)
        return self.lib.sgl_attention_probs(a["ctx"], a["B"], a["H"], a["W"], a["saved"], a["saved_bytes"], a["layer"],
                                            a["mode"], a["out"], a["out_bytes"], None)

    def close(self):
        self.lib.sgl_destroy(self.ctx)


@pytest.fixture()
def plain(pkg, hiplib):
    c = Ctx(pkg, hiplib)
    yield c
    c.close()


def test_ctx_null_pointers(plain):
    assert plain.call(ctx=None) == ah.ERR_NULL
    assert plain.call(saved=None) == ah.ERR_NULL
    assert plain.call(out=None) == ah.ERR_NULL


def test_ctx_bad_shape(plain):
    assert plain.call(B=0) == ah.ERR_BAD_SHAPE
    assert plain.call(H=13) == ah.ERR_BAD_SHAPE               # smaller than a patch
    assert plain.call(layer=-1) == ah.ERR_BAD_SHAPE
    assert plain.call(layer=plain.L + 1) == ah.ERR_BAD_SHAPE


def test_ctx_order_of_refusals(plain):
    assert plain.call(saved=None, layer=-1, mode=7, saved_bytes=0) == ah.ERR_NULL          # NULL first
    assert plain.call(layer=-1, mode=7, saved_bytes=0) == ah.ERR_BAD_SHAPE                 # then shape
    assert plain.call(mode=7, saved_bytes=0) == ah.ERR_UNSUPPORTED                         # then mode
    assert plain.call(saved_bytes=0) == ah.ERR_WORKSPACE                                   # sizes last


def test_ctx_unsupported(pkg, hiplib, plain):
    assert plain.call(mode=2) == ah.ERR_UNSUPPORTED
    assert plain.call(mode=-1) == ah.ERR_UNSUPPORTED
    for kw in (dict(recompute=1), dict(mode="mxfp8")):
        c = Ctx(pkg, hiplib, **kw)
        try:
            assert c.call() == ah.ERR_UNSUPPORTED, kw
            assert c.call(layer=c.L) == ah.ERR_UNSUPPORTED, kw
        finally:
            c.close()
    c = Ctx(pkg, hiplib, use_head=0)
    try:
        assert c.call(layer=c.L) == ah.ERR_UNSUPPORTED          # no pooling head, no probe map
        assert c.call(layer=c.L, mode=ar.HEAD_MEAN) == ah.ERR_UNSUPPORTED
    finally:
        c.close()


def test_ctx_workspace(plain):
    B, Hh, N, L = plain.B, plain.heads, plain.N, plain.L
    assert plain.call(saved_bytes=plain.saved_bytes - 1) == ah.ERR_WORKSPACE
    assert plain.call(out_bytes=B * Hh * N * N * 4 - 1) == ah.ERR_WORKSPACE
    assert plain.call(mode=ar.HEAD_MEAN, out_bytes=B * N * N * 4 - 1) == ah.ERR_WORKSPACE
    assert plain.call(layer=L, out_bytes=B * Hh * N * 4 - 1) == ah.ERR_WORKSPACE
    assert plain.call(layer=L, mode=ar.HEAD_MEAN, out_bytes=B * N * 4 - 1) == ah.ERR_WORKSPACE


# ---------------------------------------------------------------------------------------------------------------
# goldens
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_goldens_load_and_rows_sum_to_one(pkg, name):
    meta, att = load_case(name)
    cfg = pkg.get_config(str(meta["meta.config"]))
    B, H, W = int(meta["meta.batch"]), int(meta["meta.res_h"]), int(meta["meta.res_w"])
    N = (H // cfg.patch_size) * (W // cfg.patch_size)
    assert len(att) == cfg.num_hidden_layers
    for a in att:
        assert a.shape == (B, cfg.num_attention_heads, N, N) and a.dtype == torch.float32
        assert float((a.double().sum(-1) - 1).abs().max()) <= (N + 4) * ar.EPS32      # an N-term fp32 softmax row
        assert float(a.min()) >= 0.0
    pool = torch.from_numpy(meta["pooling"])
    assert pool.shape == (B, cfg.num_attention_heads, N)
    assert float((pool.double().sum(-1) - 1).abs().max()) <= (N + 4) * ar.EPS32
    for tag in ("bf16ac.", "fp16ac."):
        assert meta[tag + "attn.l2rel"].shape == (len(att),) and (meta[tag + "attn.l2rel"] > 0).all()
        assert meta[tag + "attn.maxerr"].shape == (len(att),)
        assert float(meta[tag + "pooling.l2rel"]) > 0


def test_golden_files_are_small():
    files = glob.glob(os.path.join(GOLDEN, "*.npz"))
    assert len(files) == sum(1 + int(np.load(os.path.join(GOLDEN, n + ".npz"))["meta.layers"]) for n in CASES)
    assert max(os.path.getsize(f) for f in files) < (1 << 20)


# ---------------------------------------------------------------------------------------------------------------
# heads.attention_rollout
# ---------------------------------------------------------------------------------------------------------------
def rollout64(att, residual, pooling=None):
    R = None
    for A in att:
        A = A.double()
        if A.dim() == 4:
            A = A.mean(1)
        B, N, _ = A.shape
        At = torch.empty_like(A)
        for b in range(B):
            M = (1 - residual) * A[b] + residual * torch.eye(N, dtype=torch.float64)
            At[b] = M / M.sum(-1, keepdim=True)
        R = At if R is None else torch.stack([At[b] @ R[b] for b in range(B)])
    if pooling is None:
        return R
    p = pooling.double()
    if p.dim() == 3:
        p = p.mean(1)
    return torch.stack([p[b] @ R[b] for b in range(R.shape[0])])


@pytest.mark.parametrize("name", CASES)
def test_rollout_matches_float64_loop(pkg, name):
    meta, att = load_case(name)
    roll = pkg.heads.attention_rollout
    N, L = att[0].shape[-1], len(att)
    # L products of row-stochastic N x N matrices in fp32: each entry is an N-term sum of non-negative terms
    tol = L * (N + 8) * ar.EPS32
    for residual in (0.5, 0.0, 0.9):
        got = roll(att, residual)
        assert got.dtype == torch.float32 and got.shape == (att[0].shape[0], N, N)
        ref = rollout64(att, residual)
        assert float((got.double() - ref).abs().max()) <= tol * max(1.0, float(ref.max()))
        assert float((got.double().sum(-1) - 1).abs().max()) <= tol                      # rows of a rollout sum to 1
    # head-mean inputs give the same thing as the 4-D ones
    means = [a.mean(1) for a in att]
    assert float((roll(means, 0.5).double() - rollout64(att, 0.5)).abs().max()) <= tol
    # residual = 1: the identity, exactly
    eye = torch.eye(N).expand(att[0].shape[0], N, N)
    assert torch.equal(roll(att, 1.0), eye)
    # a single layer gives its mixed, renormalised matrix
    one = roll(att[:1], 0.5)
    A = att[0].double().mean(1)
    M = 0.5 * A + 0.5 * torch.eye(N, dtype=torch.float64)
    assert float((one.double() - M / M.sum(-1, keepdim=True)).abs().max()) <= 8 * ar.EPS32
    # through the pooling head's probe attention: (B, N), a distribution over patches
    pool = torch.from_numpy(meta["pooling"])
    rel = roll(att, 0.5, pooling=pool)
    assert rel.shape == (att[0].shape[0], N)
    assert float((rel.double() - rollout64(att, 0.5, pool)).abs().max()) <= tol
    assert float((rel.double().sum(-1) - 1).abs().max()) <= 2 * tol
    assert torch.equal(roll(att, 0.5, pooling=pool.mean(1)), rel) or \
        float((roll(att, 0.5, pooling=pool.mean(1)) - rel).abs().max()) <= 4 * ar.EPS32


def test_rollout_needs_a_map(pkg):
    with pytest.raises(ValueError):
        pkg.heads.attention_rollout([])


# ---------------------------------------------------------------------------------------------------------------
# the Python surface: errors raised before any device work (the inputs are CPU tensors; nothing reaches the library)
# ---------------------------------------------------------------------------------------------------------------
def test_python_refusals(pkg):
    cfg = pkg.get_config("tiny")
    x = torch.zeros(1, 3, 32, 32)
    m = pkg.SiglipVisionModelHIP(cfg, recompute=True)
    with pytest.raises(RuntimeError, match="use a model without recompute for attention maps"):
        m(pixel_values=x, output_attentions=True)
    m = pkg.SiglipVisionModelHIP(cfg, compute_dtype="mxfp8")
    with pytest.raises(RuntimeError, match="mxfp8.*use compute_dtype='bf16'"):
        m(pixel_values=x, output_attentions=True)
    m = pkg.SiglipVisionModelHIP(cfg)
    for bad in ([3], [0, -4], [cfg.num_hidden_layers]):
        with pytest.raises(RuntimeError, match="out of range"):
            m(pixel_values=x, output_attentions=True, attention_layers=bad)
    with pytest.raises(ValueError, match="attention_heads"):
        m(pixel_values=x, output_attentions=True, attention_heads="max")
    # a valid request on a CPU tensor gets as far as the device check every forward makes, and no further
    with pytest.raises(RuntimeError, match="runs only on an AMD GPU"):
        m(pixel_values=x, output_attentions=True, attention_layers=[0, -1], attention_heads="mean")
    headless = pkg.SiglipVisionModelHIP(ah.make_config(pkg, "tiny", use_head=0))
    with pytest.raises(RuntimeError, match="pooling head"):
        headless.attention_rollout(x)


def test_output_fields_default_to_none(pkg):
    out = pkg.encoder.VisionModelOutput(last_hidden_state=torch.zeros(1), pooler_output=None)
    assert out.attentions is None and out.pooling_attention is None and out[2] is None
