"""GPU tests of the 384x192-tile NT GEMM (gemm_nt6_kernel on the NtTile384 geometry), through the C ABI (``sgl_op_gemm_nt``).

The dispatch sends an NT GEMM there when M >= 2048, N % 192 == 0, N % 256 != 0 and the epilogue is EPI_STORE, or EPI_RES_F32
with K >= 2048 (at smaller K the residual launch is bound by its memory traffic and the tile does not pay).
``SGL_NT_TILE=256|384`` (read once per process) forces one tile, so the EPI_RES_F32 cases with K < 2048 are held to the float64
bound in the child process that runs under ``SGL_NT_TILE=384``; in this process they run on whatever the dispatch picks.
Same yardstick as the 256x256 kernel's tests in tests/test_kernel_edges_gpu.py: every element against the float64 reference
with the bound of ``kernel_ref.gemm_ref``, every leading dimension 8 above the logical width with NaN in the slack, guard bands
round the output.

The kernel keeps the accumulation order of the 256x256 kernel (K-steps ascending, k-half 0 then 1, one MFMA chain per
accumulator), so on the same inputs the two tiles must agree bit for bit: two child processes (the switch is read once) run
the same launches under ``SGL_NT_TILE=256`` and ``=384`` and report a digest of every output.
"""
import hashlib
import json
import os
import subprocess
import sys

import pytest
import torch

import kernel_ref as kr
from kernel_ref import BF16, F16
from test_kernel_edges_gpu import Guarded, check_nt_epilogue, gemm_nt, lib, nt_operands, ok, padded, randn, tdt_of  # noqa: F401

pytestmark = pytest.mark.gpu
EPI_STORE, EPI_RES_F32 = 0, 2

# M: 2048 = 5 1/3 row tiles (the last one has 128 rows: wave rows 2 and 3 of it are idle), 2304 = exactly 6, 2051 ragged and odd.
# N: 2, 3 and 6 column tiles, none a multiple of 256.
# K: one, two (with a tail chunk) and two full K-steps (pipeline prologue without a loop issue), four with K % 64 != 0, and the
#    production depth (18 steps: both groups' in-loop issue and every wait).
MS, NS, KS = [2048, 2304, 2051], [384, 576, 1152], [64, 72, 128, 200, 1152]
# every (M, K), (N, K) and (M, N) pair appears: N index = (M index + K index) % 3
SHAPES = [(M, NS[(mi + ki) % 3], K) for mi, M in enumerate(MS) for ki, K in enumerate(KS)]
VARIANTS = [(BF16, EPI_STORE), (F16, EPI_STORE), (BF16, EPI_RES_F32), (F16, EPI_RES_F32)]


@pytest.mark.parametrize("dtype,epi", VARIANTS, ids=lambda v: str(v))
@pytest.mark.parametrize("M,N,K", SHAPES, ids=lambda v: str(v))
def test_nt384_fp64_bound_ld_guard(lib, M, N, K, dtype, epi):
    """EPI_STORE (bf16 / fp16 output, with bias) and EPI_RES_F32 (bias + fp32 residual, ldr = ldo = N + 8), lda = ldb = K + 8."""
    check_nt_epilogue(lib, dtype, M, N, K, epi, seed=M + N + K + epi)


def test_nt384_res_default_dispatch_fp64_bound(lib):
    """EPI_RES_F32 deep enough (K >= 2048) for the default dispatch to pick the 384x192 tile: 33 K-steps, ragged M."""
    check_nt_epilogue(lib, BF16, 2051, 576, 2112, EPI_RES_F32, seed=3)


def launch(lib, dtype, M, N, K, epi, seed):
    """One guarded launch on seeded inputs; returns the Guarded output."""
    g, A, B, bias = nt_operands(dtype, M, N, K, seed)
    odt = torch.float32 if epi == EPI_RES_F32 else tdt_of(dtype)
    out = Guarded(M, N, N + 8, odt)
    kw = {}
    if epi == EPI_RES_F32:
        kw = dict(res=padded(randn(g, M, N), N + 8), ldr=N + 8)
    ok(gemm_nt(lib, dtype, A, K + 8, B, K + 8, M, N, K, epi, out.ptr, N + 8, bias=bias, **kw))
    out.check(f"NT M={M} N={N} K={K} epi={epi}")
    return out


def bits(out):
    t = out.got().contiguous()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def digest(out):
    return hashlib.sha256(bits(out).cpu().numpy().tobytes()).hexdigest()


# launches of the child processes: name -> (dtype, M, N, K, epilogue)
AB_CASES = {
    "store_bf16": (BF16, 2051, 1152, 1152, EPI_STORE),
    "store_f16": (F16, 2048, 576, 200, EPI_STORE),
    "res_bf16": (BF16, 2051, 1152, 1152, EPI_RES_F32),
    "res_f16": (F16, 2048, 576, 200, EPI_RES_F32),
    # never sent to the 384x192 tile by the default dispatch: N divides by 256 / does not divide by 192
    "n768": (BF16, 2051, 768, 200, EPI_STORE),
    "n4352": (BF16, 2051, 4352, 72, EPI_STORE),
}


def all_digests(hl):
    return {name: digest(launch(hl, dt, M, N, K, epi, seed=17)) for name, (dt, M, N, K, epi) in AB_CASES.items()}


def tile_child():
    """Body of the child processes of `forced`: every AB_CASES launch under the SGL_NT_TILE of the environment."""
    import __graft_entry__ as entry
    hl = entry.load_package().lib.load()
    res = all_digests(hl)
    if os.environ.get("SGL_NT_TILE") == "384":   # every EPI_RES_F32 case of the module on the 384x192 tile, whatever its K
        for dtype in (BF16, F16):
            for M, N, K in SHAPES:
                check_nt_epilogue(hl, dtype, M, N, K, EPI_RES_F32, seed=M + N + K + EPI_RES_F32)
        res["res_bounds_checked"] = 2 * len(SHAPES)
    print("NT_TILE_DIGESTS " + json.dumps(res))


@pytest.fixture(scope="module")
def forced():
    """{256: digests, 384: digests}: one child process per forced tile."""
    here = os.path.dirname(os.path.abspath(__file__))
    code = (f"import sys; sys.path[:0] = [{os.path.dirname(here)!r}, {here!r}]; "
            f"import test_gemm_nt_384_gpu as t; t.tile_child()")
    res = {}
    for tile in (256, 384):
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300,
                           env=dict(os.environ, SGL_NT_TILE=str(tile)))
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("NT_TILE_DIGESTS ")]
        assert r.returncode == 0 and lines, r.stdout[-2000:] + r.stderr[-4000:]
        res[tile] = json.loads(lines[-1].split(" ", 1)[1])
    return res


@pytest.fixture(scope="module")
def default(lib):
    assert "SGL_NT_TILE" not in os.environ, "the suite runs with the default dispatch"
    return all_digests(lib)


@pytest.mark.parametrize("epi", ["store", "res"])
def test_nt384_bitwise_equal_to_256_tile(forced, default, epi):
    """Same inputs under SGL_NT_TILE=256 and =384 (and under the default dispatch): identical bits, bf16 and fp16."""
    for name in (f"{epi}_bf16", f"{epi}_f16"):
        assert forced[384][name] == forced[256][name], f"{name}: the two tiles disagree"
        assert default[name] == forced[256][name], f"{name}: the default dispatch disagrees with the 256x256 tile"


def test_nt384_dispatch_leaves_other_widths(forced, default):
    """N = 768 and N = 4352: the default dispatch gives the 256x256 kernel's bits (and so does a forced 384x192 tile)."""
    for name in ("n768", "n4352"):
        assert default[name] == forced[256][name], name
        assert forced[384][name] == forced[256][name], name


def test_nt384_res_fp64_bound_forced_tile(forced):
    """The child under SGL_NT_TILE=384 held every EPI_RES_F32 case (bf16 and fp16, all SHAPES) to the float64 bound."""
    assert forced[384]["res_bounds_checked"] == 2 * len(SHAPES)


@pytest.mark.parametrize("epi", [EPI_STORE, EPI_RES_F32], ids=["store", "res"])
def test_nt384_run_to_run_bitwise(lib, epi):
    K = 200 if epi == EPI_STORE else 2112   # deep enough for the default dispatch to pick the 384x192 tile
    a = bits(launch(lib, BF16, 2051, 1152, K, epi, seed=5))
    b = bits(launch(lib, BF16, 2051, 1152, K, epi, seed=5))
    assert torch.equal(a, b)
