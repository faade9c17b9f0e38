"""CPU (no GPU): the MX-fp8 inference mode's host surface, and known answers of the reference quantizer (tests/mx_ref.py)
that the HIP kernels are held to bit for bit on the GPU (tests/test_mxfp8_gpu.py).  No kernel is launched here."""
import copy
import ctypes as C
import os
import re

import pytest
import torch

import mx_ref

SO400M = (1152, 4304, 27, 16, 14, 27, 1e-6)
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "siglip_hip.h")


def test_dtype_code_matches_header(pkg):
    from siglip_amd import encoder
    assert encoder.COMPUTE_DTYPES["mxfp8"] == pkg.lib.SGL_DTYPE_MXFP8 == 5
    text = open(HEADER).read()
    assert re.search(r"SGL_DTYPE_MXFP8\s*=\s*5\b", text)
    assert encoder.OPERAND_DTYPE["mxfp8"] == torch.bfloat16    # the patch GEMM stays bf16
    from siglip_amd import preprocess
    assert preprocess._operand_dtype("mxfp8") == torch.bfloat16


def test_create_accepts_mxfp8_code_and_rejects_unassigned_ones(pkg, hiplib):
    """SGL_DTYPE_MXFP8 is 5; code 4 stays unassigned and, with the other unknown codes, is rejected."""
    L = pkg.lib
    ctx = hiplib.sgl_create(C.byref(L.SglConfig(*SO400M, L.SGL_DTYPE_MXFP8, 1)))
    assert ctx
    hiplib.sgl_destroy(ctx)
    for code in (4, 6, 7, -1):
        assert not hiplib.sgl_create(C.byref(L.SglConfig(*SO400M, code, 1)))


def _sizes(hiplib, L, dt, train, cfg=SO400M, B=64, res=384):
    ctx = hiplib.sgl_create(C.byref(L.SglConfig(*cfg, dt, 1)))
    assert ctx
    try:
        a, b, c = C.c_size_t(), C.c_size_t(), C.c_size_t()
        st = hiplib.sgl_query_sizes(ctx, B, res, res, train, C.byref(a), C.byref(b), C.byref(c))
        return st, (a.value, b.value, c.value)
    finally:
        hiplib.sgl_destroy(ctx)


def test_create_accepts_mxfp8_and_refuses_training(pkg, hiplib):
    L = pkg.lib
    st, _ = _sizes(hiplib, L, L.SGL_DTYPE_MXFP8, 1)
    assert st == -2    # SGL_ERR_UNSUPPORTED: the mode has no backward
    st, (sh_mx, saved, ws_mx) = _sizes(hiplib, L, L.SGL_DTYPE_MXFP8, 0)
    assert st == 0 and saved == 0
    st, (sh_bf, _, ws_bf) = _sizes(hiplib, L, L.SGL_DTYPE_BF16, 0)
    assert st == 0
    # MX blocks (1 + 1/32 bytes per weight, no transposes) against bf16 row-major + transposed copies (4 bytes per weight)
    assert 0 < sh_mx < 0.4 * sh_bf
    assert 0 < ws_mx < ws_bf
    # tiny (D = 64) and hostile (D = 144, I = 538) pad K to 128
    for cfg in ((64, 128, 2, 2, 8, 4, 1e-6), (144, 538, 2, 2, 14, 3, 1e-6)):
        st, (sh, saved, ws) = _sizes(hiplib, L, L.SGL_DTYPE_MXFP8, 0, cfg=cfg, B=2, res=42)
        assert st == 0 and sh > 0 and ws > 0


@pytest.mark.parametrize("ctor", ["model", "open_clip", "from_pretrained"])
def test_constructors_accept_mxfp8_and_deepcopy_keeps_it(pkg, ctor):
    cfg = pkg.get_config("tiny")
    if ctor == "model":
        m = pkg.SiglipVisionModelHIP(cfg, "mxfp8")
    elif ctor == "open_clip":
        m = pkg.OpenClipStyleEncoder(cfg, "mxfp8").visual
    else:
        with pytest.warns(UserWarning):
            m = pkg.SiglipVisionModelHIP.from_pretrained("tiny", compute_dtype="mxfp8", allow_random_init=True)
    assert m.compute_dtype == "mxfp8"
    assert copy.deepcopy(m).compute_dtype == "mxfp8"
    with pytest.raises(ValueError, match="mxfp8"):
        pkg.SiglipVisionModelHIP(cfg, "fp8")


def test_create_model_and_transforms_accepts_mxfp8(pkg):
    from siglip_amd import encoder
    import inspect
    assert "compute_dtype" in inspect.signature(encoder.create_model_and_transforms).parameters
    enc = pkg.OpenClipStyleEncoder(pkg.get_config("tiny"), compute_dtype="mxfp8")
    assert enc.visual.compute_dtype == "mxfp8"


# ---- the quantizer's known answers ------------------------------------------------------------------------------------
def _q(vals, K=32):
    x = torch.zeros(1, K, dtype=torch.float64)
    x[0, :len(vals)] = torch.tensor(vals, dtype=torch.float64)
    return mx_ref.quantize(x)


def test_scale_boundary_at_448():
    q, s = _q([448.0])
    assert s[0, 0].item() == 127 and q[0, 0].item() == 0x7E           # 448 = 1.75 * 2^8: the largest e4m3fn value
    q, s = _q([float(torch.nextafter(torch.tensor(448.0, dtype=torch.float32), torch.tensor(1e9)).item())])
    assert s[0, 0].item() == 128                                         # just above 448 needs 2^1
    q, s = _q([448.0 * 2 ** 5])
    assert s[0, 0].item() == 132 and q[0, 0].item() == 0x7E
    q, s = _q([256.0])                                                   # m = 1 < 1.75: e = k - 8 = 0
    assert s[0, 0].item() == 127 and q[0, 0].item() == 0x78


def test_rne_ties_to_even():
    # amax 448 -> e = 0; between 1.0 (0x38) and 1.125 (0x39) the tie 1.0625 goes to the even code 0x38,
    # between 1.125 and 1.25 (0x3A) the tie 1.1875 goes to 0x3A
    q, s = _q([448.0, 1.0625, 1.1875, -1.0625, 1.07])
    assert s[0, 0].item() == 127
    assert q[0, 1:5].tolist() == [0x38, 0x3A, 0xB8, 0x39]


def test_e4m3_subnormals_kept():
    # amax 448 -> e = 0: 2^-9 is the smallest subnormal (code 1), 3 * 2^-9 code 3, 2^-10 ties to 0, 1.5 * 2^-9 ties to 2
    q, s = _q([448.0, 2.0 ** -9, 3 * 2.0 ** -9, 2.0 ** -10, 1.5 * 2.0 ** -9, 7.5 * 2.0 ** -9])
    assert q[0, 1:6].tolist() == [1, 3, 0, 2, 8]


def test_all_zero_block_and_padding():
    x = torch.zeros(2, 40, dtype=torch.float64)
    x[1, 33] = 1.0
    q, s = mx_ref.quantize(x)
    assert q.shape == (2, 128) and s.shape == (2, 4)
    assert s[0].tolist() == [0, 0, 0, 0] and q[0].abs().sum().item() == 0
    assert s[1].tolist() == [0, 119, 0, 0]     # amax 1 = 1 * 2^0: e = -8
    assert q[1, 33].item() == 0x78            # 1 * 2^8 = 256


def test_fp32_subnormal_amax_clamps():
    tiny = float(torch.tensor(1e-40, dtype=torch.float32).item())   # an fp32 subnormal
    q, s = _q([tiny])
    assert s[0, 0].item() == 0                 # e clamps to -127
    # tiny * 2^127 ~ 1.7e-2: representable, so the element survives
    assert q[0, 0].item() != 0
    assert abs(mx_ref.dequantize(q, s)[0, 0].item() - tiny) <= 0.07 * tiny


def test_non_finite_block():
    q, s = _q([1.0, float("inf"), 2.0])
    assert s[0, 0].item() == 255 and all(v == 0x7F for v in q[0, :32].tolist())
    assert s[0, 1].item() == 0


def test_round_trip_error_is_bounded():
    torch.manual_seed(0)
    x = torch.randn(64, 256, dtype=torch.float64) * torch.logspace(-3, 3, 256, dtype=torch.float64)
    d = mx_ref.fake_quant(x)
    blk = x.reshape(64, 8, 32).abs().amax(-1, keepdim=True)
    # relative step of e4m3 is 2^-3, so half a step at the block's top binade bounds every element's error
    assert ((d - x).reshape(64, 8, 32).abs() <= blk * 2.0 ** -4 + 1e-300).all()
