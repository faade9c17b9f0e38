"""CPU (no GPU): the block-recompute policy's C ABI (sgl_create_ex, buffer sizes, training token limit) and its Python
surface (model.recompute, gradient_checkpointing_enable/disable, set_grad_checkpointing, the custom ops' fake impls).
No kernel is launched here."""
import copy
import ctypes as C
import warnings

import pytest
import torch

SO400M = (1152, 4304, 27, 16, 14, 27, 1e-6)
TINY = (64, 128, 3, 4, 4, 8, 1e-6)
HOSTILE = (144, 538, 2, 2, 14, 3, 1e-6)


def _create(hiplib, L, cfg, dt, recompute):
    return hiplib.sgl_create_ex(C.byref(L.SglConfig(*cfg, dt, 1)), recompute)


def _sizes(hiplib, ctx, B, res, train):
    a, b, c = C.c_size_t(), C.c_size_t(), C.c_size_t()
    st = hiplib.sgl_query_sizes(ctx, B, res, res, train, C.byref(a), C.byref(b), C.byref(c))
    return st, (a.value, b.value, c.value)


def _block_region(B, N, cfg=SO400M, es=2):
    """Bytes of one block's activation region (Layout: stats1, h1, qkv, attn, lse, xmid, stats2, h2, u, a)."""
    D, I, _, H = cfg[:4]
    Ip, DP, M = (I + 127) // 128 * 128, ((D // H) + 15) // 16 * 16, B * N
    parts = [M * 8, M * D * es, 3 * B * H * N * DP * es, M * D * es, B * H * N * 4, M * D * 4, M * 8, M * D * es,
             M * Ip * es, M * Ip * es]
    return sum((p + 255) // 256 * 256 for p in parts)


def test_create_ex_policies(pkg, hiplib):
    L = pkg.lib
    assert (L.SGL_RECOMPUTE_NONE, L.SGL_RECOMPUTE_BLOCKS) == (0, 1)
    for dt in (L.SGL_DTYPE_F32, L.SGL_DTYPE_BF16, L.SGL_DTYPE_BF16X3, L.SGL_DTYPE_F16):
        for rc in (0, 1):
            ctx = _create(hiplib, L, SO400M, dt, rc)
            assert ctx, (dt, rc)
            hiplib.sgl_destroy(ctx)
        for bad in (2, -1, 7):
            assert not _create(hiplib, L, SO400M, dt, bad)
    # the MX-fp8 mode never trains: nothing to recompute
    assert not _create(hiplib, L, SO400M, L.SGL_DTYPE_MXFP8, 1)
    ctx = _create(hiplib, L, SO400M, L.SGL_DTYPE_MXFP8, 0)
    assert ctx
    hiplib.sgl_destroy(ctx)


@pytest.mark.parametrize("cfg,shapes", [(SO400M, [(128, 384), (4, 384), (3, 224)]), (TINY, [(2, 32), (3, 48)]),
                                        (HOSTILE, [(2, 42), (1, 98)])])
@pytest.mark.parametrize("dt", [0, 1, 2, 3])
def test_policy_none_is_sgl_create(pkg, hiplib, cfg, shapes, dt):
    L = pkg.lib
    a = hiplib.sgl_create(C.byref(L.SglConfig(*cfg, dt, 1)))
    b = _create(hiplib, L, cfg, dt, 0)
    r = _create(hiplib, L, cfg, dt, 1)
    try:
        for B, res in shapes:
            for train in (0, 1):
                assert _sizes(hiplib, a, B, res, train) == _sizes(hiplib, b, B, res, train)
            # inference sizes and the shadow arena do not depend on the policy
            assert _sizes(hiplib, a, B, res, 0) == _sizes(hiplib, r, B, res, 0)
            st, (sh, _, _) = _sizes(hiplib, r, B, res, 1)
            assert st == 0 and sh == _sizes(hiplib, a, B, res, 1)[1][0]
    finally:
        for c in (a, b, r):
            hiplib.sgl_destroy(c)


@pytest.mark.parametrize("dt", [0, 1, 2, 3])
def test_so400m_b128_sizes(pkg, hiplib, dt):
    """saved loses the 27 per-block regions; ws gains one (the bf16x3 split scratch of the forward moves out of saved and
    reuses the backward's)."""
    L = pkg.lib
    a = _create(hiplib, L, SO400M, dt, 0)
    r = _create(hiplib, L, SO400M, dt, 1)
    try:
        st0, (sh0, sv0, ws0) = _sizes(hiplib, a, 128, 384, 1)
        st1, (sh1, sv1, ws1) = _sizes(hiplib, r, 128, 384, 1)
        assert st0 == st1 == 0 and sh0 == sh1
        es = 4 if dt in (L.SGL_DTYPE_F32, L.SGL_DTYPE_BF16X3) else 2
        region = _block_region(128, 729, es=es)
        if es == 2:
            assert region == 3_423_430_656
        split = 0
        if dt == L.SGL_DTYPE_BF16X3:   # the two split-operand buffers: [3 * M][widest row, padded to 8] bf16 each
            split = 2 * (3 * 128 * 729 * 4352 * 2)
        assert sv0 - sv1 == 27 * region + split
        assert ws1 - ws0 == region
        # memory held from forward to backward (saved + 28 fp32 hidden states + the shared region): under 0.2x
        hs = 28 * 128 * 729 * 1152 * 4
        assert (sv1 + hs + region) <= 0.2 * (sv0 + hs)
    finally:
        hiplib.sgl_destroy(a)
        hiplib.sgl_destroy(r)


@pytest.mark.parametrize("dt,limit", [(1, 493_447), (3, 493_447), (0, 246_723), (2, 164_482)])
def test_training_token_limit(pkg, hiplib, dt, limit):
    """Every context refuses shapes whose widest GEMM operand would reach 2^32 bytes (the GEMMs' 32-bit buffer ranges):
    SGL_ERR_BAD_SHAPE from sgl_query_sizes, training and inference, recompute and plain context alike."""
    L = pkg.lib
    a = _create(hiplib, L, SO400M, dt, 0)
    r = _create(hiplib, L, SO400M, dt, 1)
    try:
        bmax = limit // 729
        assert _sizes(hiplib, r, bmax, 384, 1)[0] == 0
        assert _sizes(hiplib, r, bmax + 1, 384, 1)[0] == -1
        assert _sizes(hiplib, r, bmax + 1, 384, 0)[0] == -1
        assert _sizes(hiplib, a, bmax + 1, 384, 1)[0] == -1
        # exact boundary in tokens (patch 14 on a one-patch-high image: B tokens)
        assert _sizes(hiplib, r, limit, 14, 1)[0] == 0
        assert _sizes(hiplib, r, limit + 1, 14, 1)[0] == -1
    finally:
        hiplib.sgl_destroy(a)
        hiplib.sgl_destroy(r)


def _token_limit(cfg, dt, train):
    """The token limit restated from the operands each pass hands to the GEMMs (see test_token_limit_every_context)."""
    D, I, _, _, P = cfg[:5]
    Ip, Kp = (I + 127) // 128 * 128, (3 * P * P + 63) // 64 * 64
    if dt == 5:   # MX-fp8
        return min((2 ** 32 - 1) // (2 * max(D, Kp)), 65535 * 128, 2 ** 22 - 1)
    w = max(Ip, D, Kp, 3 * D if train else 0)
    row = {0: 4 * w, 1: 2 * w, 3: 2 * w, 2: 3 * ((w + 7) // 8 * 8) * 2}[dt]
    return min((2 ** 32 - 1) // row, 2 ** 22 - 1)


# so400m: Ip = 4352 > 3 D = 3456 > Kp = 640, so the forward's widest row and the training path's are the same 4352
LIMITS = {(SO400M, 1): 493_447, (SO400M, 3): 493_447, (SO400M, 0): 246_723, (SO400M, 2): 164_482}


@pytest.mark.parametrize("train", [0, 1])
@pytest.mark.parametrize("recompute", [0, 1])
@pytest.mark.parametrize("dt", [0, 1, 2, 3])
@pytest.mark.parametrize("cfg", [SO400M, TINY, HOSTILE], ids=["so400m", "tiny", "hostile"])
def test_token_limit_every_context(pkg, hiplib, cfg, dt, recompute, train):
    """One token limit for plain and recompute contexts, inference and training: the limit is accepted, one token more is
    SGL_ERR_BAD_SHAPE, at 384 px (B = limit // 729) and token-exact on a one-patch-high image (B tokens).

    Derivation, from the operands a pass hands to gemm_nt / gemm_tn with M = B * grid rows (csrc/encoder.hip): the forward
    reads im2col [M][Kp] (patch GEMM), h1 / attn / h2 [M][D] (QKV, out_proj, fc1), a [M][Ip] (fc2) and the head's cast of the
    last hidden state [M][D]; its widest row is max(Ip, D, Kp) elements.  Training adds u / du [M][Ip] and dqkv [M][3 D]
    (dX and dW of the QKV projection): max(Ip, 3 D, Kp).  gemm_nt_mfma / gemm_tn_mfma refuse M * row_bytes >= 2^32, so
    limit = floor((2^32 - 1) / row_bytes): 2 bytes per element in bf16 / fp16, 4 in strict fp32, and the bf16x3 operand is
    [M][3 * round_up(w, 8)] bf16.  so400m: w = 4352 both ways (Ip > 3 D), hence 4294967295 // 8704 = 493 447,
    // 17408 = 246 723, // 26112 = 164 482 for inference as for training.  tiny (w = 128, 192 training) is narrow: its
    quotient is above the 2^22 - 1 rows up to which the EPI_QKV row split is exact, which is then the limit (4 194 303)
    on a plain context and on inference too, but for bf16x3 training (4294967295 // 1152 = 3 728 270).  hostile (w = 640 = Ip = Kp) lies
    between: 3 355 443 in bf16 / fp16, 1 677 721 in fp32, 1 118 481 in bf16x3."""
    L = pkg.lib
    limit = _token_limit(cfg, dt, train)
    if (cfg, dt) in LIMITS:
        assert limit == LIMITS[(cfg, dt)]
    elif cfg is TINY:
        assert limit == (3_728_270 if (dt, train) == (2, 1) else 2 ** 22 - 1)
    else:
        assert limit == {1: 3_355_443, 3: 3_355_443, 0: 1_677_721, 2: 1_118_481}[dt]
    P = cfg[4]
    ctx = _create(hiplib, L, cfg, dt, recompute)
    try:
        assert _sizes(hiplib, ctx, limit, P, train)[0] == 0
        assert _sizes(hiplib, ctx, limit + 1, P, train)[0] == -1
        res = 384 if cfg is SO400M else 27 * P          # 729 tokens per image
        bmax = limit // 729
        assert _sizes(hiplib, ctx, bmax, res, train)[0] == 0
        assert _sizes(hiplib, ctx, bmax + 1, res, train)[0] == -1
    finally:
        hiplib.sgl_destroy(ctx)


@pytest.mark.parametrize("cfg,limit", [(SO400M, 1_864_135), (TINY, 4_194_303), (HOSTILE, 3_355_443)],
                         ids=["so400m", "tiny", "hostile"])
def test_token_limit_mxfp8(pkg, hiplib, cfg, limit):
    """MX-fp8 (inference only): its own kernels index with size_t and gemm_nt_mx has no operand guard; the bound comes from
    the bf16 GEMMs it still runs, the patch GEMM's im2col [M][Kp] and the head's cast of the last hidden state [M][D]
    (so400m: 4294967295 // 2304), from gemm_nt_mx's 65 535 row tiles of 128 and from the head's EPI_QKV row split."""
    L = pkg.lib
    assert _token_limit(cfg, 5, 0) == limit
    ctx = _create(hiplib, L, cfg, L.SGL_DTYPE_MXFP8, 0)
    try:
        P = cfg[4]
        assert _sizes(hiplib, ctx, limit, P, 0)[0] == 0
        assert _sizes(hiplib, ctx, limit + 1, P, 0)[0] == -1
        assert _sizes(hiplib, ctx, limit // 729, 27 * P, 0)[0] == 0
        assert _sizes(hiplib, ctx, limit // 729 + 1, 27 * P, 0)[0] == -1
        assert _sizes(hiplib, ctx, limit, P, 1)[0] == -2            # a shape that passes: MX-fp8 has no training pass
        assert _sizes(hiplib, ctx, limit + 1, P, 1)[0] == -1        # the shape is judged first
        # the mode has no recompute context (sgl_create_ex returns NULL: test_create_ex_policies), so plain is all there is
    finally:
        hiplib.sgl_destroy(ctx)


# ---- Python surface ---------------------------------------------------------------------------------------------------
def test_recompute_property(pkg):
    cfg = pkg.get_config("tiny")
    m = pkg.SiglipVisionModelHIP(cfg)
    assert m.recompute is False
    m.recompute = True
    assert m.recompute is True
    m.recompute = False
    assert pkg.SiglipVisionModelHIP(cfg, "bf16", recompute=True).recompute is True
    assert pkg.SiglipVisionModelHIP(cfg, "fp16", True).recompute is True
    with pytest.raises(TypeError):
        m.recompute = 1
    with pytest.raises(TypeError):
        pkg.SiglipVisionModelHIP(cfg, recompute="yes")
    with pytest.raises(ValueError, match="inference-only"):
        pkg.SiglipVisionModelHIP(cfg, "mxfp8", recompute=True)
    mx = pkg.SiglipVisionModelHIP(cfg, "mxfp8")
    with pytest.raises(ValueError, match="inference-only"):
        mx.recompute = True
    with pytest.raises(ValueError):
        mx.gradient_checkpointing_enable(recompute=True)
    assert mx.recompute is False
    with pytest.warns(UserWarning, match="RANDOM"):
        m2 = pkg.SiglipVisionModelHIP.from_pretrained("tiny", allow_random_init=True, recompute=True)
    assert m2.recompute is True


def test_gradient_checkpointing_enable_disable(pkg):
    cfg = pkg.get_config("tiny")
    m = pkg.SiglipVisionModelHIP(cfg)
    # the bare call (as the reference makes it) keeps its old meaning: a warned no-op
    with pytest.warns(UserWarning, match="no-op") as rec:
        m.gradient_checkpointing_enable()
    assert "recompute=True" in str(rec[0].message)
    assert m.recompute is False
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        m.gradient_checkpointing_enable()          # warns once only
        m2 = pkg.SiglipVisionModelHIP(cfg)
        m2.gradient_checkpointing_enable(recompute=True)
        assert m2.recompute is True
        m2.gradient_checkpointing_disable()
        assert m2.recompute is False
        m2.gradient_checkpointing_enable(recompute=True)
    m2.encoder.layers[0].mlp.fc1.weight.requires_grad_(False)
    c = copy.deepcopy(m2)
    assert c.recompute is True and c is not m2
    assert not c.encoder.layers[0].mlp.fc1.weight.requires_grad
    assert copy.deepcopy(m).recompute is False


def test_open_clip_set_grad_checkpointing(pkg):
    enc = pkg.OpenClipStyleEncoder(pkg.get_config("tiny"))
    assert enc.visual.recompute is False
    enc.set_grad_checkpointing()
    assert enc.visual.recompute is True
    enc.set_grad_checkpointing(False)
    assert enc.visual.recompute is False
    enc.set_grad_checkpointing(True)
    assert enc.visual.recompute is True


def test_fake_encoder_fwd_sizes_saved_by_policy(pkg, hiplib):
    from torch._subclasses.fake_tensor import FakeTensorMode
    cfg = pkg.get_config("tiny")
    m = pkg.SiglipVisionModelHIP(cfg, "bf16")
    params = m._table.params()
    plain, rc = m._contexts.sizes(2, 32, 32, True), m._contexts.sizes(2, 32, 32, True, True)
    assert rc[1] < plain[1] and rc[2] > plain[2] and rc[0] == plain[0]
    assert m._contexts.sizes(2, 32, 32, False, True) == m._contexts.sizes(2, 32, 32, False)
    with FakeTensorMode(allow_non_fake_inputs=True):
        x = torch.empty(2, 3, 32, 32)
        old = torch.ops.siglip_hip.encoder_fwd(x, params, m._handle, True, False, True, [1, 3], 0, 0, 0, 0)   # 11 args
        off = torch.ops.siglip_hip.encoder_fwd(x, params, m._handle, True, False, True, [1, 3], 0, 0, 0, 0, False)
        on = torch.ops.siglip_hip.encoder_fwd(x, params, m._handle, True, False, True, [1, 3], 0, 0, 0, 0, True)
        inf = torch.ops.siglip_hip.encoder_fwd(x, params, m._handle, False, False, True, [], 0, 0, 0, 0, True)
    assert old[4].numel() == off[4].numel() == plain[1]
    assert on[4].numel() == rc[1]
    assert inf[2].numel() == 0                   # inference saves nothing, whatever the policy
    assert [tuple(o.shape) for o in on[:4]] == [tuple(o.shape) for o in old[:4]]
    assert tuple(on[5].shape) == tuple(old[5].shape)
