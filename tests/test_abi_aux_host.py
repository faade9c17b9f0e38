"""CPU (no GPU): every documented early return of the single-kernel entry points outside the encoder.

As in tests/test_abi_contract_host.py, each call is invalid in exactly one argument and returns BEFORE the first HIP
call; device pointers are dummy integers that are never dereferenced.  Were a check missing, the call would reach the
HIP runtime and come back as SGL_ERR_HIP on a machine without a device, so the case fails cleanly.  No valid call is made.
"""
import pytest

OK, BAD_SHAPE, UNSUPPORTED, WORKSPACE, NULL = 0, -1, -2, -3, -5
D = 0x7F0000001000          # a 16-byte aligned dummy device pointer, never dereferenced
F32, BF16, F16 = 0, 1, 3


@pytest.fixture(scope="module")
def lib(hiplib):
    return hiplib


def test_l2norm_tmean_fwd_admits_only_what_64k_of_lds_holds(lib):
    """D floats of dynamic LDS plus 16 static bytes must fit 64 KiB: 16380 * 4 + 16 = 65536.  The header's limit is 16380;
    16381 and the 16384 an earlier header admitted are refused before any launch."""
    for d in (16381, 16384, 1 << 20):
        assert d * 4 + 16 > 65536
        assert lib.sgl_op_l2norm_tmean_fwd(D, D, D, 1, 1, d, None) == BAD_SHAPE
    assert 16380 * 4 + 16 == 65536
    for b, t, d in ((0, 1, 8), (1, 0, 8), (1, 1, 0)):
        assert lib.sgl_op_l2norm_tmean_fwd(D, D, D, b, t, d, None) == BAD_SHAPE
        assert lib.sgl_op_l2norm_tmean_bwd(D, D, D, D, b, t, d, None) == BAD_SHAPE
    for k in range(3):
        a = [D, D, D]
        a[k] = None
        assert lib.sgl_op_l2norm_tmean_fwd(*a, 1, 1, 8, None) == NULL
    for k in range(4):
        a = [D, D, D, D]
        a[k] = None
        assert lib.sgl_op_l2norm_tmean_bwd(*a, 1, 1, 8, None) == NULL


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_dwconv_refuses_misaligned_pointers_and_bad_shapes(lib, dtype):
    """x, y, w9, bias (forward) and x, dy (weight gradient) are read and written with 16-byte vector accesses: a pointer
    4 or 8 bytes off is SGL_ERR_BAD_SHAPE, with no launch."""
    nv = 8 if dtype == BF16 else 4
    for off in (4, 8, 2):
        for k in range(4):
            a = [D, D, D, D]                # x, w9, bias, y
            a[k] = D + off
            assert lib.sgl_op_dwconv3x3(a[0], dtype, a[1], a[2], a[3], 1, 3, 3, 64, 0, None) == BAD_SHAPE
        for k in range(2):
            a = [D, D]                      # x, dy
            a[k] = D + off
            assert lib.sgl_op_dwconv3x3_wgrad(a[0], a[1], dtype, D, 0, D, 1 << 30, 1, 3, 3, 64, None) == BAD_SHAPE
    for E in (nv // 2, nv * 3, 1024 + nv, nv * 96):          # below one vector; 256 % 3; above 1024; 256 % 96
        assert lib.sgl_op_dwconv3x3(D, dtype, D, D, D, 1, 3, 3, E, 0, None) == BAD_SHAPE
        assert lib.sgl_op_dwconv3x3_wgrad(D, D, dtype, D, 0, D, 1 << 30, 1, 3, 3, E, None) == BAD_SHAPE
    assert lib.sgl_op_dwconv3x3(D, BF16, D, D, D, 1, 3, 3, 24, 0, None) == BAD_SHAPE        # 256 % (24 / 8) != 0
    for b, gh, gw in ((0, 3, 3), (1, 0, 3), (1, 3, 0)):
        assert lib.sgl_op_dwconv3x3(D, dtype, D, D, D, b, gh, gw, 64, 0, None) == BAD_SHAPE
    assert lib.sgl_op_dwconv3x3(D, F16, D, D, D, 1, 3, 3, 64, 0, None) == UNSUPPORTED
    assert lib.sgl_op_dwconv3x3(None, dtype, D, D, D, 1, 3, 3, 64, 0, None) == NULL
    assert lib.sgl_op_dwconv3x3(D, dtype, None, D, D, 1, 3, 3, 64, 0, None) == NULL
    assert lib.sgl_op_dwconv3x3(D, dtype, D, D, None, 1, 3, 3, 64, 0, None) == NULL
    need = 9 * 10 * 64 * 4                                   # 9 pixels -> 9 blocks of [10][E] partials
    assert lib.sgl_op_dwconv3x3_wgrad(D, D, dtype, D, 0, D, need - 1, 1, 3, 3, 64, None) == WORKSPACE
    assert lib.sgl_op_dwconv3x3_wgrad(D, D, dtype, D, 0, None, need, 1, 3, 3, 64, None) == NULL
    assert lib.sgl_op_dwconv3x3_wgrad_scratch_bytes(7, 9, 9, 64) == 512 * 10 * 64 * 4


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_gate_mul_argument_checks(lib, dtype):
    nv = 8 if dtype == BF16 else 4
    assert lib.sgl_op_gate_mul(D, D, D, nv + 1, dtype, None) == BAD_SHAPE
    assert lib.sgl_op_gate_mul_bwd(D, D, D, D, D, nv - 1, dtype, None) == BAD_SHAPE
    for k in range(3):
        a = [D, D, D]
        a[k] = D + 4
        assert lib.sgl_op_gate_mul(*a, nv * 4, dtype, None) == BAD_SHAPE
        a[k] = None
        assert lib.sgl_op_gate_mul(*a, nv * 4, dtype, None) == NULL
    for k in range(5):
        a = [D, D, D, D, D]
        a[k] = D + 8
        assert lib.sgl_op_gate_mul_bwd(*a, nv * 4, dtype, None) == BAD_SHAPE
    for k in range(3):
        a = [D, D, D, D, D]
        a[k] = None
        assert lib.sgl_op_gate_mul_bwd(*a, nv * 4, dtype, None) == NULL
    assert lib.sgl_op_gate_mul(D, D, D, 64, F16, None) == UNSUPPORTED
    assert lib.sgl_op_gate_mul(D, D, D, 0, dtype, None) == OK             # nothing to do: no launch


def test_seg_loss_shape_limits(lib):
    assert lib.sgl_op_seg_loss_chunks(42) == 6 and lib.sgl_op_seg_loss_chunks(8) == 1 and lib.sgl_op_seg_loss_chunks(0) == 0
    for b, g, s in ((0, 3, 42), (1, 0, 42), (1, 3, 0), (1, 4097, 42), (1, 3, 16385)):
        assert lib.sgl_op_seg_loss_fwd(D, D, D, b, g, s, None) == BAD_SHAPE
    for b, g, s in ((0, 3, 42), (1, 0, 42), (1, 3, 0), (1, 4097, 42), (1, 3, 8193)):
        assert lib.sgl_op_seg_loss_bwd(D, D, D, D, D, b, g, s, 1e-6, None) == BAD_SHAPE
    for k in range(3):
        a = [D, D, D]
        a[k] = None
        assert lib.sgl_op_seg_loss_fwd(*a, 1, 3, 42, None) == NULL
    for k in range(5):
        a = [D, D, D, D, D]
        a[k] = None
        assert lib.sgl_op_seg_loss_bwd(*a, 1, 3, 42, 1e-6, None) == NULL


@pytest.mark.parametrize("entry", ["sgl_op_preprocess", "sgl_op_preprocess_aug"])
def test_preprocess_argument_checks(lib, entry):
    def call(src=D, u8=1, B=2, Hs=30, Ws=30, out=D, dt=BF16, S=42, P=14, Kp=640, pm=1, mean=0.5, std=0.5, tab=D, gm=D):
        if entry == "sgl_op_preprocess":
            return lib.sgl_op_preprocess(src, u8, B, Hs, Ws, out, dt, S, P, Kp, pm, mean, std, None, 1.0, None)
        return lib.sgl_op_preprocess_aug(src, u8, B, Hs, Ws, out, dt, S, P, Kp, pm, mean, std, tab, gm, None)
    assert call(std=0.0) == BAD_SHAPE
    assert call(Kp=587) == BAD_SHAPE                  # Kp < 3 P^2
    assert call(S=13) == BAD_SHAPE                    # S < P
    assert call(P=0) == BAD_SHAPE
    assert call(B=0) == BAD_SHAPE and call(Hs=0) == BAD_SHAPE and call(Ws=0) == BAD_SHAPE and call(S=0, pm=0) == BAD_SHAPE
    assert call(src=None) == NULL and call(out=None) == NULL
    for bad in (2, 4, 5, -1):
        assert call(dt=bad) == UNSUPPORTED
    assert call(Hs=673) == UNSUPPORTED                # 673 / 42 > 16
    assert call(Ws=225, S=14, P=14) == UNSUPPORTED    # 225 / 14 > 16
    if entry == "sgl_op_preprocess_aug":
        assert call(tab=None) == NULL and call(gm=None) == NULL


def test_adamw_argument_checks(lib):
    for step in (0, -3):
        assert lib.sgl_op_adamw(D, D, 4, 0.9, 0.999, 1e-8, step, None, None) == BAD_SHAPE
        assert lib.sgl_op_adamw_ex(D, D, D, 4, 0.9, 0.999, 1e-8, step, None, None, 0, 0.0, None) == BAD_SHAPE
    assert lib.sgl_op_adamw(D, D, -1, 0.9, 0.999, 1e-8, 1, None, None) == BAD_SHAPE
    assert lib.sgl_op_adamw(None, D, 4, 0.9, 0.999, 1e-8, 1, None, None) == NULL
    assert lib.sgl_op_adamw(D, None, 4, 0.9, 0.999, 1e-8, 1, None, None) == NULL
    assert lib.sgl_op_adamw(D, D, 0, 0.9, 0.999, 1e-8, 1, None, None) == OK       # empty plan: no launch
