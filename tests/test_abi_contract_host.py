"""CPU (no GPU): every documented early return of the encoder entry points, and sgl_query_sizes as a function.

Each call below is invalid in exactly one argument and, by the code in csrc/encoder.hip, returns BEFORE the first HIP call
(argument errors are reported before any work is enqueued).  Device pointers are dummy non-null integers that are never
dereferenced; host tables (hs_slots[], layers[], d_taps[]) are real arrays.  Were a check missing, the call would reach
the HIP runtime and come back as SGL_ERR_HIP on a machine without a device, so the case fails cleanly.  No fully valid
call is made here (it would launch kernels on the dummy pointers).
"""
import ctypes as C
import itertools

import pytest

import abi_harness as ah

DUMMY = 0x7F0000001000          # never dereferenced
CFGS = {"tiny": (32, 32), "hostile": (42, 42)}


class Host:
    """One context with dummy device pointers and the real sizes of a (B, H, W) geometry."""

    def __init__(self, pkg, lib, cfg_name="hostile", mode="bf16", recompute=0, B=2, HW=None, train=True, use_head=1):
        self.pkg, self.lib = pkg, lib
        self.cfg = ah.make_config(pkg, cfg_name, use_head)
        self.L = self.cfg.num_hidden_layers
        self.ctx = lib.sgl_create_ex(C.byref(ah.sgl_config(pkg, self.cfg, mode, use_head)), recompute)
        assert self.ctx
        self.w, self._wl = ah.weights_struct(pkg, self.cfg, lambda n: DUMMY)
        Lb = pkg.lib
        self._gl = (Lb.SglLayerPtrs * max(self.L, 1))()
        for l in range(self.L):
            for f in ah.LAYER_NAMES:
                setattr(self._gl[l], f, DUMMY)
        self.g = Lb.SglGrads()
        self.g.layers = C.cast(self._gl, C.POINTER(Lb.SglLayerPtrs))
        for f in list(ah.GLOBAL_NAMES) + list(ah.HEAD_NAMES):
            setattr(self.g, f, DUMMY)
        self.B = B
        self.H, self.W = HW or CFGS[cfg_name]
        self.train = train
        a, b, c = C.c_size_t(), C.c_size_t(), C.c_size_t()
        st = lib.sgl_query_sizes(self.ctx, B, self.H, self.W, 1 if train else 0, C.byref(a), C.byref(b), C.byref(c))
        self.size_status = st
        self.shadow_bytes, self.saved_bytes, self.ws_bytes = a.value, b.value, c.value
        self.M = B * (self.H // self.cfg.patch_size) * (self.W // self.cfg.patch_size)
        self.slot = self.M * self.cfg.hidden_size * 4

    def close(self):
        self.lib.sgl_destroy(self.ctx)

    def table(self, ptrs):
        return (C.c_void_p * len(ptrs))(*ptrs)

    def defaults(self, entry):
        L, t = self.L, self.train
        saved = [("saved", DUMMY if t else None), ("saved_bytes", self.saved_bytes if t else 0)]
        tail = saved + [("ws", DUMMY), ("ws_bytes", self.ws_bytes)]
        dims = [("B", self.B), ("H", self.H), ("W", self.W)]
        fwd = [("ctx", self.ctx), ("w", C.byref(self.w)), ("shadow", DUMMY), ("pixels", DUMMY), ("channels_last", 0)] + \
            dims + [("interp", 1)]
        outs = [("last_hidden", DUMMY), ("pooled", DUMMY)]
        bwd = [("ctx", self.ctx), ("w", C.byref(self.w)), ("shadow", DUMMY), ("g", C.byref(self.g))]
        d3 = [("d_last_hidden", DUMMY), ("d_pooled", DUMMY), ("d_tap_last", None)]
        if entry == "sgl_prepare_weights":
            return [("ctx", self.ctx), ("w", C.byref(self.w)), ("shadow", DUMMY), ("shadow_bytes", self.shadow_bytes),
                    ("stream", None)]
        if entry == "sgl_prepare_weights_dirty":
            return [("ctx", self.ctx), ("w", C.byref(self.w)), ("shadow", DUMMY), ("shadow_bytes", self.shadow_bytes),
                    ("layer_dirty", None), ("globals_dirty", 1), ("stream", None)]
        if entry == "sgl_forward":
            return fwd + [("hidden_states", DUMMY), ("hs_slots", L + 1)] + outs + tail + [("stream", None)]
        if entry == "sgl_forward_ex":
            return fwd + [("hidden_states", DUMMY), ("hs_slots", L + 1)] + outs + tail + [("ftb", 0), ("stream", None)]
        if entry == "sgl_forward_slots":
            slots = self.table([DUMMY + l * self.slot for l in range(L + 1)])
            return fwd + [("hs_slots", slots)] + outs + tail + [("ftb", 0), ("stream", None)]
        if entry in ("sgl_backward_begin", "sgl_backward_begin_p"):
            return bwd + dims + [("hidden_states", DUMMY)] + d3 + tail + [("stream", None)]
        if entry in ("sgl_backward_layer", "sgl_backward_layer_p"):
            return bwd + [("layer", L - 1)] + dims + [("hidden_states", DUMMY), ("d_tap", None), ("need_dx", 1)] + tail + \
                [("stream", None)]
        if entry == "sgl_backward_embed":
            return [("ctx", self.ctx), ("w", C.byref(self.w)), ("g", C.byref(self.g))] + dims + [("interp", 1)] + tail + \
                [("stream", None)]
        if entry == "sgl_backward":
            return bwd + dims + [("interp", 1), ("hidden_states", DUMMY), ("d_taps", None), ("d_last_hidden", DUMMY),
                                 ("d_pooled", DUMMY), ("ftb", 0), ("train_embeddings", 1)] + tail + [("stream", None)]
        raise KeyError(entry)

    def call(self, entry, **over):
        args = self.defaults(entry)
        names = [n for n, _ in args]
        for k in over:
            assert k in names, (entry, k)
        return getattr(self.lib, entry)(*[over.get(n, v) for n, v in args])


FORWARDS = ["sgl_forward", "sgl_forward_ex", "sgl_forward_slots"]
BACKWARDS = ["sgl_backward_begin", "sgl_backward_begin_p", "sgl_backward_layer", "sgl_backward_layer_p",
             "sgl_backward_embed", "sgl_backward"]
PREPARES = ["sgl_prepare_weights", "sgl_prepare_weights_dirty"]


@pytest.fixture
def host(pkg, hiplib):
    made = []

    def make(*a, **kw):
        made.append(Host(pkg, hiplib, *a, **kw))
        return made[-1]
    yield make
    for h in made:
        h.close()


@pytest.mark.parametrize("mode", ["fp32", "bf16", "bf16x3", "fp16", "mxfp8"])
def test_arena_one_byte_short_is_err_workspace(host, mode):
    trains = mode != "mxfp8"
    h = host("hostile", mode, 0, train=trains)
    for e in PREPARES:
        assert h.call(e, shadow_bytes=h.shadow_bytes - 1) == ah.ERR_WORKSPACE, e
    hi = host("hostile", mode, 0, train=False)                 # inference: the activations live in ws
    for e in FORWARDS:
        assert hi.call(e, ws_bytes=hi.ws_bytes - 1) == ah.ERR_WORKSPACE, e
    if not trains:
        return
    for e in FORWARDS:                                          # plain training forward: saved
        assert h.call(e, saved_bytes=h.saved_bytes - 1) == ah.ERR_WORKSPACE, e
    for e in BACKWARDS:
        assert h.call(e, saved_bytes=h.saved_bytes - 1) == ah.ERR_WORKSPACE, e
        assert h.call(e, ws_bytes=h.ws_bytes - 1) == ah.ERR_WORKSPACE, e
    r = host("hostile", mode, 1, train=True)                    # recompute: the training forward needs ws as well
    for e in FORWARDS:
        assert r.call(e, saved_bytes=r.saved_bytes - 1) == ah.ERR_WORKSPACE, e
        assert r.call(e, ws_bytes=r.ws_bytes - 1) == ah.ERR_WORKSPACE, e
    for e in BACKWARDS:
        assert r.call(e, saved_bytes=r.saved_bytes - 1) == ah.ERR_WORKSPACE, e
        assert r.call(e, ws_bytes=r.ws_bytes - 1) == ah.ERR_WORKSPACE, e


@pytest.mark.parametrize("recompute", [0, 1])
@pytest.mark.parametrize("cfg_name", ["tiny", "hostile"])
def test_required_pointer_null_is_err_null(host, pkg, cfg_name, recompute):
    h = host(cfg_name, "bf16", recompute, train=True)
    L = h.L
    no_layers = pkg.lib.SglWeights()
    C.memmove(C.byref(no_layers), C.byref(h.w), C.sizeof(no_layers))
    no_layers.layers = None
    no_glayers = pkg.lib.SglGrads()
    C.memmove(C.byref(no_glayers), C.byref(h.g), C.sizeof(no_glayers))
    no_glayers.layers = None
    for e in PREPARES:
        for arg in ("ctx", "w", "shadow"):
            assert h.call(e, **{arg: None}) == ah.ERR_NULL, (e, arg)
        assert h.call(e, w=C.byref(no_layers)) == ah.ERR_NULL, (e, "w->layers")
    for e in FORWARDS:
        hs = "hs_slots" if e == "sgl_forward_slots" else "hidden_states"
        for arg in ("ctx", "w", "shadow", "pixels", hs, "last_hidden"):
            assert h.call(e, **{arg: None}) == ah.ERR_NULL, (e, arg)
        assert h.call(e, w=C.byref(no_layers)) == ah.ERR_NULL, (e, "w->layers")
    for l in range(L + 1):                                       # one NULL entry of the slot table
        ptrs = [DUMMY + k * h.slot for k in range(L + 1)]
        ptrs[l] = None
        assert h.call("sgl_forward_slots", hs_slots=h.table(ptrs)) == ah.ERR_NULL, l
    if recompute:                                               # a recompute training forward needs the workspace
        for e in FORWARDS:
            assert h.call(e, ws=None) == ah.ERR_NULL, (e, "ws")
    hi = host(cfg_name, "bf16", recompute, train=False)
    for e in FORWARDS:                                          # so does inference
        assert hi.call(e, ws=None) == ah.ERR_NULL, (e, "ws")
    for e in BACKWARDS:
        args = ["ctx", "w", "g", "saved", "ws"]
        if e != "sgl_backward_embed":
            args += ["shadow", "hidden_states"]
        for arg in args:
            assert h.call(e, **{arg: None}) == ah.ERR_NULL, (e, arg)
    for e in ("sgl_backward_layer", "sgl_backward_layer_p", "sgl_backward"):
        assert h.call(e, g=C.byref(no_glayers)) == ah.ERR_NULL, (e, "g->layers")
        assert h.call(e, w=C.byref(no_layers)) == ah.ERR_NULL, (e, "w->layers")
    # sgl_backward with a d_taps table: the host array is read (entries may be NULL), the error is still reported first
    taps = h.table([None] * (L + 1))
    assert h.call("sgl_backward", d_taps=taps, saved=None) == ah.ERR_NULL


@pytest.mark.parametrize("cfg_name", ["tiny", "hostile"])
def test_bad_shapes_are_err_bad_shape(host, cfg_name):
    h = host(cfg_name, "bf16", 0, train=True)
    hi = host(cfg_name, "bf16", 0, train=False)
    L, P = h.L, h.cfg.patch_size
    for e in ("sgl_forward", "sgl_forward_ex"):
        for n in (1, 0, -3):
            assert hi.call(e, hs_slots=n) == ah.ERR_BAD_SHAPE, (e, n)
        for n in range(2, L + 1):                               # saved != NULL needs every hidden state
            assert h.call(e, hs_slots=n) == ah.ERR_BAD_SHAPE, (e, n)
    for a, b in itertools.combinations(range(L + 1), 2):        # training: the slots must be distinct buffers
        ptrs = [DUMMY + k * h.slot for k in range(L + 1)]
        ptrs[b] = ptrs[a]
        assert h.call("sgl_forward_slots", hs_slots=h.table(ptrs)) == ah.ERR_BAD_SHAPE, (a, b)
    for e in ("sgl_backward_layer", "sgl_backward_layer_p"):
        for layer in (-1, L, L + 7):
            assert h.call(e, layer=layer) == ah.ERR_BAD_SHAPE, (e, layer)
    for e in FORWARDS + BACKWARDS:
        hh = hi if e in FORWARDS else h
        assert hh.call(e, B=0) == ah.ERR_BAD_SHAPE, e
        assert hh.call(e, B=-2) == ah.ERR_BAD_SHAPE, e
        assert hh.call(e, H=P - 1) == ah.ERR_BAD_SHAPE, e
        assert hh.call(e, W=P - 1) == ah.ERR_BAD_SHAPE, e
    # a non-native grid needs interpolate_pos (square and rectangular; a rectangular grid with the native token count too)
    g0 = h.cfg.native_grid
    for gh, gw in ((g0 + 1, g0 + 1), (g0, g0 + 1), (g0 * g0, 1)):
        hn = host(cfg_name, "bf16", 0, HW=(gh * P, gw * P), train=False)
        ht = host(cfg_name, "bf16", 0, HW=(gh * P + 3, gw * P + 1), train=True)
        for e in FORWARDS:
            assert hn.call(e, interp=0) == ah.ERR_BAD_SHAPE, (e, gh, gw)
            assert ht.call(e, interp=0) == ah.ERR_BAD_SHAPE, (e, gh, gw)


# The pooling head keeps one fp32 partial per 8-column chunk of every token of an image in the 64 KiB LDS window
# (csrc/kernels.h pool_attn_max_tokens; the kernels are in csrc/attention_pool.hip): N <= floor(16376 / (DP / 8 + 1))
# forward, floor(16376 / (DP / 8 + 2)) backward.
# hostile: head dimension 72, DP 80 (so400m's), patch 14 -> 1488 / 1364 tokens; tiny: head dimension 16, DP 16, patch 16
# -> 5458 / 4094.  (grid, train, accepted): squares either side of each limit, then rectangles just over it (and one exactly at it).
POOL_LIMIT_CASES = {
    "hostile": [((36, 36), 1, True), ((37, 37), 1, False), ((37, 37), 0, True), ((38, 38), 0, True), ((39, 39), 0, False),
                ((36, 38), 1, False), ((35, 39), 1, False), ((31, 44), 1, True), ((36, 38), 0, True),
                ((38, 40), 0, False), ((10, 149), 0, False), ((31, 48), 0, True), ((1, 1489), 0, False)],
    "tiny": [((63, 63), 1, True), ((64, 64), 1, False), ((64, 64), 0, True), ((73, 73), 0, True), ((74, 74), 0, False),
             ((63, 65), 1, False), ((46, 89), 1, True), ((53, 103), 0, False), ((2, 2729), 0, True)],
}


@pytest.mark.parametrize("mode,recompute", [("bf16", 0), ("fp32", 1)])
@pytest.mark.parametrize("cfg_name", ["hostile", "tiny"])
def test_pool_head_token_limit_is_err_bad_shape_before_any_launch(host, cfg_name, mode, recompute):
    """504 / 518 / 532 / 546 px for hostile (= so400m's head): sgl_query_sizes and every forward / backward entry point refuse
    an image whose token count the pooling head cannot hold, with SGL_ERR_BAD_SHAPE and without a device.  An accepted
    shape passes the shape check (shown by the NEXT check failing: one byte of workspace short).  use_head = 0: no limit."""
    P = {"hostile": 14, "tiny": 16}[cfg_name]
    lim = {"hostile": (1488, 1364), "tiny": (5458, 4094)}[cfg_name]
    if cfg_name == "hostile":
        assert [(g[0] * P, t, a) for g, t, a in POOL_LIMIT_CASES[cfg_name][:5]] == \
            [(504, 1, True), (518, 1, False), (518, 0, True), (532, 0, True), (546, 0, False)]
    for (gh, gw), train, accepted in POOL_LIMIT_CASES[cfg_name]:
        assert accepted == (gh * gw <= lim[train]), (gh, gw, train)            # the table agrees with the formula
        for use_head in (1, 0):
            h = host(cfg_name, mode, recompute, B=1, HW=(gh * P + 3, gw * P), train=bool(train), use_head=use_head)
            want_ok = accepted or not use_head
            what = (cfg_name, gh, gw, train, use_head)
            assert h.size_status == (ah.OK if want_ok else ah.ERR_BAD_SHAPE), what
            entries = FORWARDS + (BACKWARDS if train else [])
            for e in entries:
                if want_ok:
                    short = dict(saved_bytes=h.saved_bytes - 1) if train else dict(ws_bytes=h.ws_bytes - 1)
                    assert h.call(e, **short) == ah.ERR_WORKSPACE, (e,) + what
                else:
                    assert h.call(e) == ah.ERR_BAD_SHAPE, (e,) + what
                    assert h.call(e, ws_bytes=1 << 40, saved_bytes=(1 << 40) if train else 0) == ah.ERR_BAD_SHAPE, \
                        (e,) + what
            if not train and use_head:     # a backward at a shape only the forward accepts is refused as well
                hb = host(cfg_name, mode, recompute, B=1, HW=(gh * P, gw * P), train=True, use_head=1)
                if gh * gw > lim[1]:
                    assert hb.size_status == ah.ERR_BAD_SHAPE, what
                    for e in BACKWARDS:
                        assert hb.call(e, ws_bytes=1 << 40, saved_bytes=1 << 40) == ah.ERR_BAD_SHAPE, (e,) + what


def test_mxfp8_refuses_training(host, pkg, hiplib):
    hi = host("hostile", "mxfp8", 0, train=False)
    assert host("hostile", "mxfp8", 0, train=True).size_status == ah.ERR_UNSUPPORTED
    big = 1 << 40
    for e in FORWARDS:                                          # saved != NULL asks for a training forward
        assert hi.call(e, saved=DUMMY, saved_bytes=big, ws_bytes=big) == ah.ERR_UNSUPPORTED, e
    for e in BACKWARDS:
        assert hi.call(e, saved=DUMMY, saved_bytes=big, ws_bytes=big) == ah.ERR_UNSUPPORTED, e


def _sizes(lib, ctx, B, H, W, train):
    a, b, c = C.c_size_t(), C.c_size_t(), C.c_size_t()
    st = lib.sgl_query_sizes(ctx, B, H, W, train, C.byref(a), C.byref(b), C.byref(c))
    return st, a.value, b.value, c.value


# sgl_create_ex refuses mxfp8 with a recompute policy (tests/test_recompute_host.py), so that pair is not in the sweep
@pytest.mark.parametrize("mode,recompute", [(m, r) for m in ["fp32", "bf16", "bf16x3", "fp16", "mxfp8"] for r in (0, 1)
                                            if not (m == "mxfp8" and r)])
@pytest.mark.parametrize("cfg_name", ["tiny", "hostile", "so400m-1layer"])
def test_query_sizes_is_a_monotone_function_of_batch_and_tokens(pkg, hiplib, cfg_name, mode, recompute):
    cfg = ah.make_config(pkg, cfg_name)
    P = cfg.patch_size
    ctx = hiplib.sgl_create_ex(C.byref(ah.sgl_config(pkg, cfg, mode)), recompute)
    assert ctx
    try:
        grids = [(1, 1), (1, 2), (2, 2), (3, 2), (2, 5), (4, 3), (12, 12), (24, 6), (6, 24), (13, 12), (27, 27)]
        grids.sort(key=lambda g: g[0] * g[1])
        for train in ((0,) if mode == "mxfp8" else (0, 1)):
            prev_b = None
            for B in range(1, 6):
                prev_n, row = None, []
                for gh, gw in grids:
                    s = _sizes(hiplib, ctx, B, gh * P, gw * P, train)
                    assert s == _sizes(hiplib, ctx, B, gh * P, gw * P, train) and s[0] == ah.OK
                    # trailing pixels beyond the last whole patch do not count
                    assert s == _sizes(hiplib, ctx, B, gh * P + P - 1, gw * P + 1, train)
                    if not train:
                        assert s[2] == 0
                    if prev_n is not None:      # non-decreasing in the token count
                        assert s[2] >= prev_n[2] and s[3] >= prev_n[3] and s[1] == prev_n[1], (B, gh, gw)
                    prev_n = s
                    row.append(s)
                if prev_b is not None:          # non-decreasing in B
                    for s, q in zip(row, prev_b):
                        assert s[2] >= q[2] and s[3] >= q[3] and s[1] == q[1], B
                prev_b = row
                # Layout depends on (gh, gw) only through N: 24x6 and 6x24 patches report what 12x12 reports
                by = dict(zip(grids, row))
                assert by[(24, 6)] == by[(12, 12)] == by[(6, 24)]
    finally:
        hiplib.sgl_destroy(ctx)
