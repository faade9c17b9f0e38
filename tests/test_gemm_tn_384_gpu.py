"""GPU tests of the TN (dW) GEMM on the 384x192 tile (gemm_tn6_kernel on the NtTile384 geometry), and of both TN tiles on
grids with fewer row tiles than column tiles and the reverse, through the C ABI (``sgl_op_gemm_tn`` / ``sgl_op_gemm_tn_ws``).

``tn_plan`` (csrc/kernels.h) sends a TN GEMM to the 384x192 tile only where that tile allows more splits of the token
reduction than the 256x256 one (tiles x splits <= 256 binds: >= 11 Ki tokens at 1152 x 1152), so at test sizes the default
dispatch picks it for one case here (14,336 tokens) and every other case runs in a child process under ``SGL_TN_TILE=384``
(read once per process).  Same yardstick as the 256x256 kernel's tests in tests/test_kernel_edges_gpu.py (``check_tn``): every
element against the float64 reference with the bound of ``kernel_ref.gemm_tn_ref``, the leading dimensions above the logical
widths with NaN in the operands' slack, guard bands round the output, store and accumulate onto a non-zero matrix.

The kernel keeps the accumulation order of the 256x256 tile (K-steps ascending, k-half 0 then 1, one MFMA chain per
accumulator) and at these reduction lengths both tiles get the same split boundaries (Mred / 1024 splits: the 1024-row floor
binds, not the tile count), so on the same inputs the two tiles must agree bit for bit: two child processes run the same
launches under ``SGL_TN_TILE=256`` and ``=384`` and report a digest of every output.
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
from test_kernel_edges_gpu import DEV, Guarded, P, check_tn, gen, lib, ok, padded, randn, rup, stream, tdt_of  # noqa: F401

pytestmark = pytest.mark.gpu

# Mred: 2048 = two splits of 16 K-steps, 2115 not a multiple of the K-step (zero-filled tail rows), 4133 four splits with a tail.
# (N1, N2) on the 384x192 tile: 3 x 6 full tiles; 1.5 row tiles (wave rows 2 and 3 of the last one idle); 2 x 3 full tiles;
# ragged last column tile (520 = 2 x 192 + 136: one wave column half full); ragged last row tile (520 = 384 + 136).
MREDS = [2048, 2115, 4133]
NS = [(1152, 1152), (576, 1152), (768, 576), (1152, 520), (520, 1152)]
SLAB_WS = 32 << 20          # holds the four slabs of every case here: the deterministic slab path
CASES = [(Mred, N1, N2) for Mred in MREDS for N1, N2 in NS]
ORDER_NS = [(520, 1300), (1300, 520)]   # fewer row tiles than column tiles, and the reverse (the unit walk of a split is tile2-fastest)


def run_case(hl, dtype, Mred, N1, N2, accumulate):
    return check_tn(hl, dtype, Mred, N1, N2, accumulate=accumulate, ws_bytes=SLAB_WS, seed=Mred + N1 + 3 * N2)


@pytest.mark.parametrize("accumulate", [0, 1], ids=["store", "accumulate_onto_nonzero"])
@pytest.mark.parametrize("dtype", [BF16, F16], ids=lambda d: kr.DT_NAME[d])
@pytest.mark.parametrize("Mred,N1,N2", CASES, ids=lambda v: str(v))
def test_tn_fp64_bound_ld_guard_default_dispatch(lib, Mred, N1, N2, dtype, accumulate):
    """Every case of the module on whatever tile the default dispatch picks (the child under SGL_TN_TILE=384 runs them on
    the 384x192 tile: test_tn384_fp64_bound_forced_tile)."""
    run_case(lib, dtype, Mred, N1, N2, accumulate)


@pytest.mark.parametrize("name,ws_bytes", [("slabs_14_splits", 80 << 20), ("smaller_scratch_12_splits", 64 << 20),
                                           ("no_scratch_atomics", None)], ids=lambda v: str(v))
@pytest.mark.parametrize("accumulate", [0, 1], ids=["store", "accumulate_onto_nonzero"])
def test_tn384_default_dispatch_fp64_bound(lib, name, ws_bytes, accumulate):
    """14,336 tokens at 1152 x 1152: the default dispatch picks the 384x192 tile (18 tiles x 14 splits of 1024 rows against
    25 tiles x 10 splits of 1472).  With 64 MiB of scratch the best plan that fits is 12 splits on the same tile, still
    through slabs; without scratch the 14 splits add with atomics."""
    check_tn(lib, BF16, 14336, 1152, 1152, accumulate=accumulate, ws_bytes=ws_bytes, seed=29)


def launch(hl, dtype, Mred, N1, N2, accumulate, ws_bytes, seed):
    """One guarded launch on seeded inputs; returns the Guarded output."""
    g = gen(seed)
    tdt = tdt_of(dtype)
    lda, ldb, ldo = rup(N1, 8) + 8, rup(N2, 8) + 8, rup(N2, 4) + 4
    A = padded(randn(g, Mred, N1).to(tdt), lda)
    B = padded(randn(g, Mred, N2).to(tdt), ldb)
    out = Guarded(N1, N2, ldo, torch.float32, prior=randn(g, N1, N2) * 3 if accumulate else None)
    ws = torch.empty(max(ws_bytes, 16), device=DEV, dtype=torch.uint8)
    ok(hl.sgl_op_gemm_tn_ws(dtype, P(A), lda, P(B), ldb, Mred, N1, N2, 1, out.ptr, ldo, accumulate, P(ws), ws_bytes,
                            stream()))
    out.check(f"TN Mred={Mred} N1={N1} N2={N2}")
    return out


def digest(out):
    return hashlib.sha256(out.got().contiguous().view(torch.int32).cpu().numpy().tobytes()).hexdigest()


# launches of the child processes: name -> (dtype, Mred, N1, N2, accumulate); all through slabs (atomics have no fixed order)
AB_CASES = {
    "full_bf16": (BF16, 4133, 1152, 1152, 0),
    "full_f16_acc": (F16, 2115, 1152, 1152, 1),
    "idle_wave_rows_bf16": (BF16, 2048, 576, 1152, 0),
    "ragged_cols_f16": (F16, 4133, 1152, 520, 0),
    "ragged_rows_bf16_acc": (BF16, 2115, 520, 1152, 1),
    "six_tiles_bf16": (BF16, 2048, 768, 576, 0),
}


def all_digests(hl):
    return {name: digest(launch(hl, dt, Mred, N1, N2, acc, SLAB_WS, seed=17))
            for name, (dt, Mred, N1, N2, acc) in AB_CASES.items()}


def tile_child():
    """Body of the child processes of `forced`: every AB_CASES launch under the SGL_TN_TILE of the environment."""
    import __graft_entry__ as entry
    hl = entry.load_package().lib.load()
    res = all_digests(hl)
    if os.environ.get("SGL_TN_TILE") == "384":   # every case of the module on the 384x192 tile: slabs, and atomics once per shape
        n = 0
        for dtype in (BF16, F16):
            for accumulate in (0, 1):
                for Mred, N1, N2 in CASES:
                    run_case(hl, dtype, Mred, N1, N2, accumulate)
                    n += 1
        for N1, N2 in NS:   # scratch too small for two slabs: fp32 atomics from the 384x192 tile
            check_tn(hl, BF16, 4133, N1, N2, accumulate=1, ws_bytes=4096, seed=N1 + N2)
            check_tn(hl, F16, 2115, N1, N2, accumulate=0, ws_bytes=4096, seed=N1 + N2)
            n += 2
        for N1, N2 in ORDER_NS:   # 2 x 7 and 4 x 3 tiles of 384 x 192
            check_tn(hl, BF16, 2048, N1, N2, accumulate=0, ws_bytes=SLAB_WS, seed=N1)
            n += 1
        res["bounds_checked"] = n
    print("TN_TILE_DIGESTS " + json.dumps(res))


N_CHILD_BOUNDS = 4 * len(CASES) + 2 * len(NS) + len(ORDER_NS)


@pytest.fixture(scope="module")
def forced():
    """{256: digests, 384: digests}: one child process per forced tile."""
    here = os.path.dirname(os.path.abspath(__file__))
    code = (f"import sys; sys.path[:0] = [{os.path.dirname(here)!r}, {here!r}]; "
            f"import test_gemm_tn_384_gpu as t; t.tile_child()")
    res = {}
    for tile in (256, 384):
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300,
                           env=dict(os.environ, SGL_TN_TILE=str(tile)))
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("TN_TILE_DIGESTS ")]
        assert r.returncode == 0 and lines, r.stdout[-2000:] + r.stderr[-4000:]
        res[tile] = json.loads(lines[-1].split(" ", 1)[1])
    return res


def test_tn384_fp64_bound_forced_tile(forced):
    """The child under SGL_TN_TILE=384 held every case (bf16 and fp16, store and accumulate, slabs; atomics per shape) to
    the float64 bound with intact guard bands."""
    assert forced[384]["bounds_checked"] == N_CHILD_BOUNDS


@pytest.mark.parametrize("name", sorted(AB_CASES))
def test_tn384_bitwise_equal_to_256_tile(forced, name):
    """Same inputs, same split boundaries, under SGL_TN_TILE=256 and =384: identical bits."""
    assert forced[384][name] == forced[256][name], f"{name}: the two tiles disagree"


def test_tn_default_dispatch_is_the_256_tile_here(forced, lib):
    """At these sizes tn_plan keeps the 256x256 tile (equal splits, smaller tile area): the default dispatch gives its bits."""
    assert "SGL_TN_TILE" not in os.environ, "the suite runs with the default dispatch"
    got = all_digests(lib)
    assert got == {n: forced[256][n] for n in AB_CASES}


# Unit -> (split, tile1, tile2) on grids of both aspect ratios; the placement must not reach the output bits.
@pytest.mark.parametrize("N1,N2", ORDER_NS, ids=["fewer_row_tiles", "fewer_col_tiles"])
@pytest.mark.parametrize("dtype", [BF16, F16], ids=lambda d: kr.DT_NAME[d])
def test_tn_unit_order_fp64_bound_and_bitwise_repeat(lib, dtype, N1, N2):
    """3 x 6 and 6 x 3 tiles of 256 x 256 (2 x 7 and 4 x 3 of 384 x 192 in the child under SGL_TN_TILE=384), two splits: each
    to the float64 bound, and bit-identical between two runs."""
    check_tn(lib, dtype, 2048, N1, N2, accumulate=1, ws_bytes=SLAB_WS, seed=N1)
    a = launch(lib, dtype, 2048, N1, N2, 0, SLAB_WS, seed=7).got().contiguous().view(torch.int32)
    b = launch(lib, dtype, 2048, N1, N2, 0, SLAB_WS, seed=7).got().contiguous().view(torch.int32)
    assert torch.equal(a, b)
