"""CPU (no GPU): the fp16 compute mode's host surface and its yardstick fixtures.

``compute_dtype="fp16"`` is the bf16 mode with fp16 MFMA operands and fp16 weight shadows: same buffers, same sizes, same
kernels.  Its parity bar is the error the REAL HF model makes under fp16 autocast, stored by tests/gen_golden_fp16ac.py
under ``fp16ac.*`` in tests/golden/fp16ac/*.npz.  No kernel is launched here."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import golden_util as gu

FP16_DIR = os.path.join(gu.GOLDEN_DIR, "fp16ac")
SO400M = (1152, 4304, 27, 16, 14, 27, 1e-6)


def test_create_accepts_fp16_and_rejects_unknown(pkg, hiplib):
    L = pkg.lib
    assert L.SGL_DTYPE_F16 == 3
    ctx = hiplib.sgl_create(C.byref(L.SglConfig(*SO400M, L.SGL_DTYPE_F16, 1)))
    assert ctx
    hiplib.sgl_destroy(ctx)
    assert not hiplib.sgl_create(C.byref(L.SglConfig(*SO400M, 7, 1)))
    assert not hiplib.sgl_create(C.byref(L.SglConfig(*SO400M, 4, 1)))


@pytest.mark.parametrize("train", [1, 0])
def test_fp16_sizes_equal_bf16_sizes(pkg, hiplib, train):
    """Same 2-byte operands and shadows: the fp16 ctx needs exactly the bf16 ctx's shadow / saved / workspace bytes."""
    L = pkg.lib
    sizes = {}
    for dt in (L.SGL_DTYPE_BF16, L.SGL_DTYPE_F16):
        ctx = hiplib.sgl_create(C.byref(L.SglConfig(*SO400M, dt, 1)))
        assert ctx
        a, b, c = C.c_size_t(), C.c_size_t(), C.c_size_t()
        assert hiplib.sgl_query_sizes(ctx, 64, 384, 384, train, C.byref(a), C.byref(b), C.byref(c)) == 0
        sizes[dt] = (a.value, b.value, c.value)
        hiplib.sgl_destroy(ctx)
    assert sizes[L.SGL_DTYPE_F16] == sizes[L.SGL_DTYPE_BF16]
    assert sizes[L.SGL_DTYPE_F16][0] > 0


def test_fp16_models_construct(pkg):
    cfg = pkg.get_config("tiny")
    m = pkg.SiglipVisionModelHIP(cfg, "fp16")
    assert m.compute_dtype == "fp16"
    enc = pkg.OpenClipStyleEncoder(cfg, "fp16")
    assert enc.visual.compute_dtype == "fp16"
    with pytest.raises(ValueError):
        pkg.SiglipVisionModelHIP(cfg, "fp8")


def test_fp16_operand_dtype_map(pkg):
    import torch
    from siglip_amd import encoder, preprocess
    assert encoder.OPERAND_DTYPE["fp16"] == torch.float16
    assert encoder.COMPUTE_DTYPES["fp16"] == pkg.lib.SGL_DTYPE_F16
    assert preprocess._operand_dtype("fp16") == torch.float16
    assert pkg.lib.dtype_code(torch.float16) == pkg.lib.SGL_DTYPE_F16 == 3
    assert pkg.lib.dtype_code(torch.float32) == pkg.lib.SGL_DTYPE_F32 == 0
    assert pkg.lib.dtype_code(torch.bfloat16) == pkg.lib.SGL_DTYPE_BF16 == 1
    # the existing modes keep their operand dtypes
    assert preprocess._operand_dtype("bf16") == torch.bfloat16
    assert preprocess._operand_dtype("bf16x3") == torch.float32 and preprocess._operand_dtype("fp32") == torch.float32
    with pytest.raises(ValueError):
        pkg.lib.dtype_code(torch.float64)


@pytest.mark.parametrize("case", gu.CASES)
def test_fp16_fixtures_cover_every_bf16_entry(case):
    """Every bf16ac.* statistic of the golden case has a finite fp16ac.* twin, and HF under fp16 autocast is at least 4x
    more accurate than under bf16 autocast on the pooled output (checks the fixtures themselves)."""
    rec = gu.load(case)
    f16 = dict(np.load(os.path.join(FP16_DIR, case + ".npz")))
    keys = [k for k in rec if k.startswith("bf16ac.") and k.endswith((".maxerr", ".l2rel"))]
    assert keys
    for k in keys:
        t = "fp16ac." + k[len("bf16ac."):]
        assert t in f16, t
        assert math.isfinite(float(f16[t])), t
    assert math.isfinite(float(f16["fp16ac.loss"]))
    assert gu.meta(f16) == gu.meta(rec)
    for stat in ("l2rel", "maxerr"):
        k = f"pooler_output.{stat}"
        assert float(f16["fp16ac." + k]) <= 0.25 * float(rec["bf16ac." + k]), (case, k)


def test_full_depth_fixture():
    rec = dict(np.load(os.path.join(FP16_DIR, "so400m27_384.npz")))
    m = gu.meta(rec)
    assert m["config"] == "so400m-patch14-384" and m["batch"] == 1 and m["res"] == 384 and m["taps"] == (13, 26)
    prefixes = [k[:-len(".shape")] for k in rec if k.endswith(".shape")]
    assert {"pooler_output", "last_hidden_state", "hidden_states.13", "hidden_states.26"} <= set(prefixes)
    assert sum(p.startswith("grad.") for p in prefixes) == 8
    for p in prefixes:
        for tag in ("fp16ac.", "bf16ac."):
            for stat in (".maxerr", ".l2rel"):
                assert math.isfinite(float(rec[tag + p + stat])), tag + p + stat
    for stat in (".l2rel", ".maxerr"):
        assert float(rec["fp16ac.pooler_output" + stat]) <= 0.25 * float(rec["bf16ac.pooler_output" + stat])
