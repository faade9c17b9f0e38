"""CPU (no GPU): the contract around d loss / d pixel_values.

* every fixture of tests/golden/pixgrad (the real HF model's input gradient) against the oracle's autograd gradient, at
  the bar tests/test_oracle_golden.py holds the oracle's parameter gradients to, the uncovered border exactly zero;
* the new symbols are declared and exported; sgl_abi_version() is still 3;
* every documented early return of sgl_backward_embed_px / sgl_query_input_grad_bytes comes back before the first HIP call
  (the method of tests/test_abi_contract_host.py: dummy pointers, a machine without a device);
* the fake encoder_bwd returns a d_pixels of the input's shape and memory format;
* sgl_query_sizes reports what the commit before these entry points reported (committed table).
"""
import ctypes as C
import json

import pytest
import torch

import abi_harness as ah
import gen_query_sizes_table as qs
import golden_util as gu
import pixgrad_util as pg
from test_abi_contract_host import DUMMY, Host

NEW_SYMBOLS = ["sgl_backward_embed_px", "sgl_query_input_grad_bytes", "sgl_op_col2im"]


@pytest.mark.parametrize("case", pg.CASES)
def test_oracle_pixel_gradient_matches_hf_fixture(case, pkg, oracle):
    rec = pg.load(case)
    m = gu.meta(rec)
    cfg = pkg.get_config(m["config"])
    sd = pkg.weights.seeded_state_dict(cfg, seed=m["seed"])
    H, W = m["res_h"], m["res_w"]
    x = pkg.weights.seeded_pixels(m["batch"], H, W, seed=m["seed"] + 1000).requires_grad_(True)
    torch.set_num_threads(8)
    out = oracle.vision_forward(x, sd, cfg, True, m["interp"])
    loss = oracle.probe_loss(out, m["taps"])
    assert abs(loss.item() - float(rec["loss"])) <= 1e-3 * max(1.0, abs(float(rec["loss"])))
    loss.backward()
    assert tuple(x.grad.shape) == (m["batch"], 3, H, W)
    err, scale = gu.compare(rec, pg.PREFIX, x.grad, 2e-4, 2e-4)      # the oracle bar for gradients
    _, l2 = gu.err_stats(rec, pg.PREFIX, x.grad)
    print(f"[{case}] oracle vs HF d_pixels: max|err| {err:.2e} on scale {scale:.2e}, rel-L2 {l2:.2e}")
    # the 'valid' convolution never reads the trailing rows / columns: exactly zero in HF and in the oracle
    assert float(rec["border.absmax"]) == 0.0
    mask = pg.border_mask(m["batch"], H, W, cfg.patch_size)
    assert bool((x.grad[mask] == 0).all())
    if case in pg.EDGE_CASES:
        assert mask.any() and H % cfg.patch_size and W % cfg.patch_size
    # the autocast yardsticks the GPU tests divide by are there and sane
    for tag in ("bf16ac.", "fp16ac."):
        assert 0 < float(rec[tag + pg.PREFIX + ".l2rel"]) < 0.1 and float(rec[tag + pg.PREFIX + ".maxerr"]) > 0
    assert float(rec["fp16ac." + pg.PREFIX + ".l2rel"]) < float(rec["bf16ac." + pg.PREFIX + ".l2rel"])


def test_full_depth_fixture_shares_the_inputs_of_the_fp16ac_one():
    a, b = pg.load(pg.FULL_CASE), gu.load("fp16ac/" + pg.FULL_CASE)
    for k in ("meta.config", "meta.seed", "meta.batch", "meta.interp"):
        assert str(a[k]) == str(b[k]), k
    assert int(a["meta.res_h"]) == int(b["meta.res"]) == int(a["meta.res_w"])
    assert list(a["meta.taps"]) == list(b["meta.taps"])
    assert abs(float(a["loss"]) - float(b["loss"])) <= 1e-6 * abs(float(b["loss"]))


def test_new_symbols_are_declared_and_exported(pkg, hiplib):
    declared = pkg.lib.declared_symbols()
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert getattr(hiplib, s).argtypes is not None, s          # bound with a signature by lib.load()
    assert hiplib.sgl_abi_version() == 3                            # new symbols only


class PxHost(Host):
    def defaults(self, entry):
        if entry == "sgl_backward_embed_px":
            n = C.c_size_t()
            st = self.lib.sgl_query_input_grad_bytes(self.ctx, self.B, self.H, self.W, C.byref(n))
            self.px_bytes = n.value if st == ah.OK else 1 << 40
            return [("ctx", self.ctx), ("w", C.byref(self.w)), ("g", C.byref(self.g)), ("B", self.B), ("H", self.H),
                    ("W", self.W), ("interp", 1), ("d_pixels", DUMMY), ("channels_last", 0), ("px_scratch", DUMMY),
                    ("px_scratch_bytes", self.px_bytes), ("saved", DUMMY), ("saved_bytes", self.saved_bytes),
                    ("ws", DUMMY), ("ws_bytes", self.ws_bytes), ("stream", None)]
        return super().defaults(entry)


@pytest.fixture
def host(pkg, hiplib):
    made = []

    def make(*a, **kw):
        made.append(PxHost(pkg, hiplib, *a, **kw))
        return made[-1]
    yield make
    for h in made:
        h.close()


E = "sgl_backward_embed_px"


@pytest.mark.parametrize("recompute", [0, 1])
@pytest.mark.parametrize("mode", ah.TRAIN_MODES)
def test_embed_px_early_returns(host, pkg, mode, recompute):
    h = host("hostile", mode, recompute, B=3, HW=(101, 59), train=True)
    P = h.cfg.patch_size
    for arg in ("ctx", "w", "g", "d_pixels", "px_scratch", "saved", "ws"):
        assert h.call(E, **{arg: None}) == ah.ERR_NULL, arg
    no_patch = pkg.lib.SglWeights()
    C.memmove(C.byref(no_patch), C.byref(h.w), C.sizeof(no_patch))
    no_patch.patch_w = None                                         # the master the transposed operand is cast from
    assert h.call(E, w=C.byref(no_patch)) == ah.ERR_NULL
    # the entry's own pointers are checked first: they win over a bad shape and a short arena
    assert h.call(E, d_pixels=None, B=0) == ah.ERR_NULL
    assert h.call(E, px_scratch=None, ws_bytes=0) == ah.ERR_NULL
    assert h.call(E, channels_last=2) == ah.ERR_UNSUPPORTED         # a ready patch operand has no pixels
    assert h.call(E, channels_last=-1) == ah.ERR_UNSUPPORTED
    for over in (dict(B=0), dict(B=-2), dict(H=P - 1), dict(W=P - 1)):
        assert h.call(E, **over) == ah.ERR_BAD_SHAPE, over
    assert h.call(E, saved_bytes=h.saved_bytes - 1) == ah.ERR_WORKSPACE
    assert h.call(E, ws_bytes=h.ws_bytes - 1) == ah.ERR_WORKSPACE
    assert h.px_bytes > 0
    assert h.call(E, px_scratch_bytes=h.px_bytes - 1) == ah.ERR_WORKSPACE     # the status a short workspace gets
    assert h.call(E, px_scratch_bytes=0) == ah.ERR_WORKSPACE
    # a frozen encoder: all three embedding destinations NULL is a valid call (not made here: it would launch kernels),
    # so NULL destinations must not turn a short scratch into another status
    frozen = pkg.lib.SglGrads()
    frozen.layers = h.g.layers
    assert h.call(E, g=C.byref(frozen), px_scratch_bytes=h.px_bytes - 1) == ah.ERR_WORKSPACE


def test_query_input_grad_bytes_contract(host, pkg, hiplib):
    n = C.c_size_t(12345)
    for mode in ah.TRAIN_MODES:
        for rc in (0, 1):
            h = host("hostile", mode, rc, B=3, HW=(101, 59), train=True)
            q = lambda *a: hiplib.sgl_query_input_grad_bytes(*a)
            assert q(None, 3, 101, 59, C.byref(n)) == ah.ERR_NULL
            assert q(h.ctx, 3, 101, 59, None) == ah.ERR_NULL
            for B, H, W in ((0, 101, 59), (-1, 101, 59), (3, 13, 59), (3, 101, 13)):
                assert q(h.ctx, B, H, W, C.byref(n)) == ah.ERR_BAD_SHAPE
            assert n.value == 12345                                 # untouched by every refused call
            m = C.c_size_t()
            assert q(h.ctx, 3, 101, 59, C.byref(m)) == ah.OK
            # d_cols [M][Kp] fp32 + W_patch^T [Kp][D] in the compute dtype, each rounded up to 256 bytes
            M, Kp, D = 3 * 7 * 4, 640, h.cfg.hidden_size
            es = 2 if mode in ("bf16", "fp16") else 4
            r256 = lambda v: (v + 255) // 256 * 256
            assert m.value == r256(M * Kp * 4) + r256(Kp * D * es)
            k = C.c_size_t()                                        # trailing pixels do not count; policy does not matter
            assert q(h.ctx, 3, 98, 56, C.byref(k)) == ah.OK and k.value == m.value
    hm = host("hostile", "mxfp8", 0, train=False)
    assert hiplib.sgl_query_input_grad_bytes(hm.ctx, 2, 42, 42, C.byref(n)) == ah.ERR_UNSUPPORTED
    big = 1 << 40                                                   # the status its other backward entry points return
    assert hm.call(E, saved=DUMMY, saved_bytes=big, ws_bytes=big, px_scratch_bytes=big) == ah.ERR_UNSUPPORTED


def test_recompute_token_limit_applies(host, hiplib):
    """so400m in bf16 on a recompute context trains on at most 493 447 tokens: B = 676 at 384 px (siglip_hip.h); so does a plain context."""
    h = host("so400m-1layer", "bf16", 1, B=676, HW=(384, 384), train=True)
    n = C.c_size_t()
    assert h.size_status == ah.OK
    assert hiplib.sgl_query_input_grad_bytes(h.ctx, 676, 384, 384, C.byref(n)) == ah.OK
    assert hiplib.sgl_query_input_grad_bytes(h.ctx, 677, 384, 384, C.byref(n)) == ah.ERR_BAD_SHAPE
    assert h.call(E, B=677, saved_bytes=1 << 50, ws_bytes=1 << 50, px_scratch_bytes=1 << 50) == ah.ERR_BAD_SHAPE
    plain = host("so400m-1layer", "bf16", 0, B=676, HW=(384, 384), train=True)
    assert hiplib.sgl_query_input_grad_bytes(plain.ctx, 676, 384, 384, C.byref(n)) == ah.OK
    assert hiplib.sgl_query_input_grad_bytes(plain.ctx, 677, 384, 384, C.byref(n)) == ah.ERR_BAD_SHAPE   # one limit for all


@pytest.mark.parametrize("channels_last", [False, True])
@pytest.mark.parametrize("frozen", [False, True])
def test_fake_encoder_bwd_returns_d_pixels(pkg, frozen, channels_last):
    from torch._subclasses.fake_tensor import FakeTensorMode
    cfg = pkg.get_config("tiny")
    m = pkg.SiglipVisionModelHIP(cfg, "bf16")
    if frozen:
        m.requires_grad_(False)
    params = m._table.params()
    needs = [p.requires_grad for p in params]
    chunks, _ = m._grads.layout(needs)
    assert (len(chunks) == 0) == frozen                             # a frozen encoder has no gradient chunk at all
    B, H, W = 2, 37, 45
    with FakeTensorMode(allow_non_fake_inputs=True):
        x = torch.empty(B, 3, H, W)
        outs = torch.ops.siglip_hip.encoder_fwd(x, params, m._handle, True, True, True, [1, 3], 0, 0, 0, 0)
        taps, saved, rest = list(outs[2:4]), outs[4], outs[5]
        grads = [torch.empty(B, 64), None, None, None]
        plain = torch.ops.siglip_hip.encoder_bwd(grads, taps, saved, rest, params, m._handle, [H, W], True, True, [1, 3],
                                                 needs, False)
        got = torch.ops.siglip_hip.encoder_bwd(grads, taps, saved, rest, params, m._handle, [H, W], True, True, [1, 3],
                                               needs, False, True, channels_last)
        hs_only = torch.ops.siglip_hip.encoder_bwd([None, torch.empty(B, 4, 64)], [], saved, torch.empty(4, B * 4, 64),
                                                   params, m._handle, [H, W], True, True, [], needs, False, True, False)
    assert len(plain) == len(chunks) and len(got) == len(chunks) + 1
    for a, (total, _, _) in zip(got, chunks):
        assert tuple(a.shape) == (total,)
    d = got[-1]
    assert tuple(d.shape) == (B, 3, H, W) and d.dtype == torch.float32
    fmt = torch.channels_last if channels_last else torch.contiguous_format
    assert d.is_contiguous(memory_format=fmt)
    assert tuple(hs_only[-1].shape) == (B, 3, H, W)                 # B from hs_rest when there is no tap


def test_query_sizes_unchanged_against_the_parent_table(pkg, hiplib):
    # Two entries of the table were changed by hand when the token limit became one for every context and pass:
    # large-patch16-384 / bf16x3 inference at B = 128, 384 x 1152 (221 184 tokens; split operand [M][3 * 4096] bf16 of
    # 5.4e9 bytes, which the GEMM refuses mid-call) on the plain and the recompute context, from sizes to SGL_ERR_BAD_SHAPE.
    with open(qs.OUT) as f:
        parent = json.load(f)
    now = qs.sweep(pkg, hiplib)
    assert len(parent) > 2000 and set(now) == set(parent)
    moved = [k for k in parent if parent[k] != now[k]]
    assert not moved, f"{len(moved)} sgl_query_sizes results moved, e.g. {moved[0]}: {parent[moved[0]]} -> {now[moved[0]]}"


def test_reducer_accepts_the_empty_chunk_list_of_a_frozen_encoder(pkg):
    """A frozen encoder with a GradBucketReducer attached hands it no chunk: backward_node([]) inside an autograd pass,
    then finish(), and the end-of-pass callback, must all be no-ops."""
    red = pkg.GradBucketReducer()
    seen = []

    class Node(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return x * 2

        @staticmethod
        def backward(ctx, g):
            seen.append(red.backward_node([]))
            red.finish()
            return g * 2

    x = torch.ones(3, requires_grad=True)
    Node.apply(x).sum().backward()
    assert seen == [True] and red._pass is None and not red._pending
    assert torch.equal(x.grad, torch.full((3,), 2.0))
    m = pkg.SiglipVisionModelHIP(pkg.get_config("tiny"), "bf16").requires_grad_(False)
    m.set_grad_reducer(red)
    chunks, groups = m._grads.layout([False] * len(m._table.params()))
    assert chunks == [] and groups == {} and m._grads.buffers(chunks, m._table.params(), torch.device("cpu")) == []
