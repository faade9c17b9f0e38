"""Ragged batches, everything that needs no GPU: the refusals of sgl_query_sizes_ragged / sgl_forward_ragged in their
documented order (each is a status code returned before any launch: on a machine without a GPU a launch would be a HIP
error), the workspace sizes, the Python refusals and the output helpers."""
import ctypes as C
import re

import pytest
import torch

import abi_harness as ah

CFG = "hostile"          # patch 14, D 144, I 538 -> 640, heads 2 x 72 (pad 80), L 2
FAKE = 0x10000           # a non-NULL "device pointer": every call here is refused before anything could read it
NEW_SYMBOLS = ["sgl_query_sizes_ragged", "sgl_forward_ragged", "sgl_op_attn_fwd_varlen", "sgl_op_pool_attn_fwd_varlen",
               "sgl_op_seg_offsets"]
POOL_LIMIT = 1488        # pool_attn_max_tokens(80, 0): the pooling head's forward limit at head_dim_pad 80


class Ctx:
    def __init__(self, pkg, lib, mode="bf16", recompute=0, use_head=1):
        self.lib = lib
        self.cfg = ah.make_config(pkg, CFG, use_head)
        self.ctx = lib.sgl_create_ex(C.byref(ah.sgl_config(pkg, self.cfg, mode, use_head)), recompute)
        assert self.ctx
        self.L = self.cfg.num_hidden_layers
        # a weights struct with a layers array: the entry point looks at w->layers before anything else of it
        self.w, self._layers = ah.weights_struct(pkg, self.cfg, lambda name: FAKE)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.lib.sgl_destroy(self.ctx)

    def query(self, grids):
        n = C.c_size_t(0)
        flat = (C.c_int * (2 * max(len(grids), 1)))(*[v for g in grids for v in g])
        return self.lib.sgl_query_sizes_ragged(self.ctx, flat, len(grids), C.byref(n)), n.value

    def forward(self, grid_list, ws_bytes=0, **null):
        """sgl_forward_ragged on fake pointers; an argument named with =True is passed as NULL, slot=l nulls one entry."""
        grids = grid_list
        flat = (C.c_int * (2 * max(len(grids), 1)))(*[v for g in grids for v in g])
        slots = (C.c_void_p * (self.L + 1))(*[None if null.get("slot") == l else FAKE for l in range(self.L + 1)])
        arg = lambda name, value: None if null.get(name) else value
        return self.lib.sgl_forward_ragged(arg("ctx", self.ctx), arg("w", C.byref(self.w)), arg("shadow", FAKE),
                                           arg("patches", FAKE), arg("grids", flat), len(grids), arg("hs_slots", slots),
                                           arg("last_hidden", FAKE), FAKE, arg("ws", FAKE), ws_bytes, None)


def test_new_symbols_are_declared_and_exported(pkg, hiplib):
    header = open(pkg.lib.HEADER_PATH).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in the header"
        assert getattr(hiplib, name).argtypes is not None, f"{name} has no binding"
    assert hiplib.sgl_abi_version() == 3


def test_forward_ragged_refusals_in_order(pkg, hiplib):
    ok_grids = [(2, 2), (7, 3)]
    with Ctx(pkg, hiplib) as c:
        # 1. a NULL pointer wins over a bad shape and over a workspace that is too small
        for name in ("ctx", "w", "shadow", "patches", "grids", "hs_slots", "last_hidden", "ws"):
            assert c.forward([], 0, **{name: True}) == ah.ERR_NULL, name
        c.w.layers = None
        assert c.forward(ok_grids) == ah.ERR_NULL
        c.w.layers = C.cast(c._layers, C.POINTER(pkg.lib.SglLayerPtrs))
        # 2. the shape, before the slot table's entries and before the workspace
        assert c.forward([], 0, slot=1) == ah.ERR_BAD_SHAPE                       # S < 1
        for bad in ([(2, 2), (0, 3)], [(2, 2), (3, -1)]):
            assert c.forward(bad, 0, slot=1) == ah.ERR_BAD_SHAPE                  # a grid side < 1
        limit = (2 ** 32 - 1) // (640 * 2)          # the header's token limit: rows of 640 bf16 (I and 3 p^2, both padded)
        many = [(38, 38)] * (limit // 1444 + 1)                                   # each within the head's limit, T above
        assert c.forward(many, 0, slot=1) == ah.ERR_BAD_SHAPE
        assert c.forward([(39, 39)], 0, slot=1) == ah.ERR_BAD_SHAPE               # 1521 tokens > the pooling head's 1488
        # 3. a NULL entry of the slot table, before the workspace
        assert c.forward(ok_grids, 0, slot=c.L) == ah.ERR_NULL
        # 4. the workspace
        st, need = c.query(ok_grids)
        assert st == ah.OK and need > 0
        assert c.forward(ok_grids, need - 1) == ah.ERR_WORKSPACE
        assert c.forward(many[:-1], 0) == ah.ERR_WORKSPACE                        # T at the limit is a valid shape
    with Ctx(pkg, hiplib, use_head=0) as c:                                       # without the head no per-image limit
        assert c.query([(39, 39)])[0] == ah.OK
        assert c.forward([(39, 39)], 0) == ah.ERR_WORKSPACE


def test_query_sizes_ragged_refusals(pkg, hiplib):
    with Ctx(pkg, hiplib) as c:
        n = C.c_size_t()
        flat = (C.c_int * 2)(2, 2)
        assert c.lib.sgl_query_sizes_ragged(None, flat, 1, C.byref(n)) == ah.ERR_NULL
        assert c.lib.sgl_query_sizes_ragged(c.ctx, None, 1, C.byref(n)) == ah.ERR_NULL
        assert c.lib.sgl_query_sizes_ragged(c.ctx, flat, 1, None) == ah.OK
        assert c.query([])[0] == ah.ERR_BAD_SHAPE
        assert c.query([(0, 1)])[0] == ah.ERR_BAD_SHAPE
        assert c.query([(1, POOL_LIMIT)])[0] == ah.OK
        assert c.query([(1, POOL_LIMIT + 1)])[0] == ah.ERR_BAD_SHAPE
    # strict fp32: the reference attention keeps one image's scores in LDS, which bounds max_n (head-less: no pool limit)
    with Ctx(pkg, hiplib, mode="fp32", use_head=0) as c:
        assert c.query([(1, 4096)])[0] == ah.OK
        assert c.query([(1, 20000)])[0] == ah.ERR_BAD_SHAPE


# every context there is: the inference-only mode has no recompute context
CONTEXTS = [(m, r) for m in ("bf16", "fp16", "fp32", "bf16x3") for r in (0, 1)] + [("mxfp8", 0)]


@pytest.mark.parametrize("mode,recompute", CONTEXTS, ids=[f"{m}-rc{r}" for m, r in CONTEXTS])
def test_sizes_follow_the_fixed_layout(pkg, hiplib, mode, recompute):
    with Ctx(pkg, hiplib, mode, recompute) as c:
        prev = 0
        for gh, gw in [(1, 1), (2, 2), (3, 3), (7, 3), (15, 9), (27, 27), (38, 38)]:
            st, n = c.query([(gh, gw)])
            assert st == ah.OK
            ws = C.c_size_t()
            assert c.lib.sgl_query_sizes(c.ctx, 1, gh * 14, gw * 14, 0, None, None, C.byref(ws)) == ah.OK
            assert n == ws.value + 256, f"S = 1 at {gh}x{gw}: the fixed inference workspace plus the 256 bytes of cu"
            assert n >= prev, "the workspace shrank as T grew"
            prev = n
        # S images: never below what the same T needs as one image, and growing with every image added
        sizes = [c.query([(3, 3)] * s)[1] for s in (1, 2, 3, 64, 65)]
        assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes)


def test_op_refusals(hiplib):
    lib = hiplib
    lens = (C.c_int * 3)(4, 0, 9)
    assert lib.sgl_op_seg_offsets(None, 3, FAKE, None) == ah.ERR_NULL
    assert lib.sgl_op_seg_offsets(lens, 3, None, None) == ah.ERR_NULL
    assert lib.sgl_op_seg_offsets(lens, 0, FAKE, None) == ah.ERR_BAD_SHAPE
    assert lib.sgl_op_seg_offsets((C.c_int * 2)(4, -1), 2, FAKE, None) == ah.ERR_BAD_SHAPE
    assert lib.sgl_op_seg_offsets((C.c_int * 2)(2 ** 31 - 1, 1), 2, FAKE, None) == ah.ERR_BAD_SHAPE
    attn = lambda dtype, S, T, max_n, H, dh, DP, q=FAKE, cu=FAKE: lib.sgl_op_attn_fwd_varlen(
        dtype, q, FAKE, FAKE, FAKE, FAKE, cu, S, T, max_n, H, dh, DP, None)
    assert attn(1, 2, 10, 5, 2, 72, 80, q=None) == ah.ERR_NULL
    assert attn(1, 2, 10, 5, 2, 72, 80, cu=None) == ah.ERR_NULL
    for bad in ((0, 10, 5, 2, 72, 80), (2, 0, 5, 2, 72, 80), (2, 10, 0, 2, 72, 80), (2, 10, 5, 0, 72, 80),
                (2, 10, 5, 2, 96, 80), (2, 10, 5, 2, 72, 96), (2, 10, 5, 2, 12, 16)):
        assert attn(1, *bad) == ah.ERR_BAD_SHAPE, bad
    assert attn(0, 2, 10, 20000, 2, 72, 80) == ah.ERR_BAD_SHAPE           # strict fp32: max_n scores do not fit the LDS
    assert attn(7, 2, 10, 5, 2, 72, 80) == ah.ERR_UNSUPPORTED             # no such dtype
    assert attn(1, 2, 10, 5, 2, 72, 80, q=FAKE + 2) == ah.ERR_UNSUPPORTED  # 16-bit operands are fetched 16 bytes at a time
    pool = lambda S, T, max_n, H, dh, DP, q=FAKE: lib.sgl_op_pool_attn_fwd_varlen(
        1, q, FAKE, FAKE, FAKE, FAKE, FAKE, S, T, max_n, H, dh, DP, None)
    assert pool(2, 10, 5, 2, 72, 80, q=None) == ah.ERR_NULL
    assert pool(0, 10, 5, 2, 72, 80) == ah.ERR_BAD_SHAPE
    assert pool(2, 10, 5, 2, 70, 80) == ah.ERR_BAD_SHAPE
    assert pool(2, 4000, POOL_LIMIT + 1, 2, 72, 80) == ah.ERR_UNSUPPORTED   # the LDS window is sized by max_n


def test_python_refusals(pkg):
    cfg = pkg.get_config(CFG)
    model = pkg.SiglipVisionModelHIP(cfg)
    x = torch.zeros(3, 28, 28)
    with pytest.raises(RuntimeError, match="encoder parameter requires a gradient.*one call per image size"):
        model.forward_ragged([x])
    model.requires_grad_(False)
    with pytest.raises(RuntimeError, match="input image requires a gradient.*one call per image size"):
        model.forward_ragged([x, x.clone().requires_grad_(True)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.forward_ragged([x])
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        model.train().requires_grad_(True).forward_ragged([x])
    for bad in (torch.zeros(2, 3, 28, 28), [], [torch.zeros(2, 3, 28, 28)], [torch.zeros(3, 13, 28)], [torch.zeros(28, 28)]):
        with pytest.raises(ValueError):
            model.forward_ragged(bad)


def test_output_helpers(pkg):
    grids = ((2, 3), (1, 1), (4, 2))
    cu = (0, 6, 7, 15)
    t = torch.arange(15 * 5, dtype=torch.float32).view(15, 5)
    out = pkg.RaggedVisionModelOutput(last_hidden_state=t, pooler_output=None, grids=grids, cu_seqlens=cu)
    parts = out.unpack(t)
    assert [p.shape[0] for p in parts] == [6, 1, 8]
    assert torch.equal(torch.cat(parts), t)
    assert parts[2].data_ptr() == t[7:].data_ptr(), "unpack returns views"
    g2 = out.token_grid(t, 2)
    assert g2.shape == (4, 2, 5) and torch.equal(g2[3, 1], t[7 + 3 * 2 + 1])
    assert out.token_grid(t, 0).shape == (2, 3, 5)
    with pytest.raises(ValueError):
        out.unpack(t[:14])
