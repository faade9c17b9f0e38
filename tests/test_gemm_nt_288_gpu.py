"""GPU tests of the 256x288-tile NT GEMM (gemm_nt6_kernel on the NtTile288 geometry), through the C ABI (``sgl_op_gemm_nt``).

The dispatch sends an NT GEMM there when the epilogue is the QKV scatter (EPI_QKV) with a 16-bit output, M >= 2048,
head_dim == 72 stored 80 wide, N == 3 * heads * 72 and N % 288 == 0: a tile is four whole heads, and the epilogue walks its
chunks head by head (store_tile_qkv_heads).  ``SGL_NT_TILE=256|288`` (read once per process) forces one tile; under 288 a QKV
scatter the tile cannot take is refused.

Same yardstick as tests/test_gemm_nt_384_gpu.py and the QKV case of tests/test_kernel_edges_gpu.py: every element against
the float64 reference with the bound of ``kernel_ref.gemm_ref``, lda = ldb = K + 8 with NaN in the slack, guard rows round the
[3][B][H][tokens][80] output, the pad columns exactly +0.

The kernel keeps the accumulation order of the 256x256 kernel (K-steps ascending, k-half 0 then 1, one MFMA chain per
accumulator) and the epilogue's arithmetic ((acc + bias), rounded to nearest), so on the same inputs the two tiles must agree
bit for bit: two child processes (the switch is read once) run the same launches under ``SGL_NT_TILE=256`` and ``=288`` and
report a digest of every output.
"""
import hashlib
import json
import os
import subprocess
import sys

import pytest
import torch

import kernel_ref as kr
import nonfinite_util as nf
from kernel_ref import BF16, F16
from test_kernel_edges_gpu import Guarded, gemm_nt, lib, nt_operands, ok, padded, run_gemm_nt_qkv, tdt_of  # noqa: F401

pytestmark = pytest.mark.gpu
EPI_QKV = 3
HD, HDP = 72, 80
SGL_ERR_UNSUPPORTED = -2

# heads: N = 864 is 3 column tiles (one each of q, k, v), N = 3456 is 12.
# batch x tokens: 3 x 729 = 2187 has image boundaries inside a 64-row staging pass and a ragged last row tile (139 rows),
#   32 x 64 = 2048 is exact passes with an image boundary at every pass, 7 x 293 = 2051 is odd M (3 rows in the last tile).
# K: one K-step, a tail chunk, two full K-steps (pipeline prologue without a loop issue), ragged K, the production depth.
HEADS, BT, KS = [4, 16], [(3, 729), (32, 64), (7, 293)], [64, 72, 128, 200, 1152]
# every (batch x tokens, K), (heads, K) and (batch x tokens, heads) pair appears: heads index = (bt index + K index) % 2
SHAPES = [(b, t, HEADS[(bi + ki) % 2], K) for bi, (b, t) in enumerate(BT) for ki, K in enumerate(KS)]


def launch_qkv(hl, dtype, batch, tokens, heads, K, seed, hd=HD, hdp=HDP, expect=0):
    """One guarded EPI_QKV launch on seeded inputs, K free of the model width; returns (Guarded output, A, B, bias)."""
    M, N = batch * tokens, 3 * heads * hd
    _, A, B, bias = nt_operands(dtype, M, N, K, seed)
    out = Guarded(3 * batch * heads * tokens, hdp, hdp, tdt_of(dtype))
    st = gemm_nt(hl, dtype, A, K + 8, B, K + 8, M, N, K, EPI_QKV, out.ptr, 0, bias=bias, tokens=tokens, heads=heads, hd=hd,
                 hdp=hdp, batch=batch)
    torch.cuda.synchronize()
    assert st == expect, f"C ABI status {st}, expected {expect}"
    return out, A, B, bias


def check_qkv(hl, dtype, batch, tokens, heads, K, seed, hd=HD, hdp=HDP):
    out, A, B, bias = launch_qkv(hl, dtype, batch, tokens, heads, K, seed, hd, hdp)
    tdt = tdt_of(dtype)
    M, N = batch * tokens, 3 * heads * hd
    what = f"QKV {kr.DT_NAME[dtype]} B={batch} T={tokens} H={heads} hd={hd}/{hdp} K={K}"
    out.check(what)
    ref, bound, _ = kr.gemm_ref(A[:, :K], B[:, :K], K, kr.UNIT[tdt], [bias[None, :].expand(M, N)], kr.TINY[tdt])
    perm = lambda t: t.view(batch, tokens, 3, heads, hd).permute(2, 0, 3, 1, 4)
    got = out.got().view(3, batch, heads, tokens, hdp)
    worst = kr.assert_within(got[..., :hd], perm(ref), perm(bound), what)
    if hdp > hd:
        pad = got[..., hd:].contiguous().view(torch.int16)
        assert bool((pad == 0).all()), f"{what}: pad columns must be written as +0"
    return worst


@pytest.mark.parametrize("dtype", [BF16, F16], ids=lambda d: kr.DT_NAME[d])
@pytest.mark.parametrize("batch,tokens,heads,K", SHAPES, ids=lambda v: str(v))
def test_nt288_fp64_bound_ld_guard(lib, batch, tokens, heads, K, dtype):
    """EPI_QKV on the 256x288 tile (default dispatch): float64 bound on every element, guard rows, pad columns +0."""
    check_qkv(lib, dtype, batch, tokens, heads, K, seed=batch + tokens + heads + K)


# launches of the child processes: name -> (dtype, batch, tokens, heads, K)
AB_CASES = {
    "bf16_k1152": (BF16, 3, 729, 16, 1152),
    "f16_k1152": (F16, 3, 729, 4, 1152),
    "bf16_k200": (BF16, 3, 729, 4, 200),
    "f16_k200": (F16, 3, 729, 16, 200),
}
# EPI_QKV launches the 256x288 tile cannot take (M >= 2048, N >= 256): name -> (batch, tokens, heads, hd, hdp)
NOT_288 = {
    "hd40": (7, 300, 4, 40, 48),
    "hdp72": (7, 300, 4, 72, 72),
    "heads6": (7, 300, 6, 72, 80),       # N = 1296 = 4.5 tiles
}


def digest(out):
    return hashlib.sha256(out.got().contiguous().view(torch.int16).cpu().numpy().tobytes()).hexdigest()


def all_digests(hl):
    res = {}
    for name, (dt, b, t, h, K) in AB_CASES.items():
        out = launch_qkv(hl, dt, b, t, h, K, seed=17)[0]
        out.check(name)
        res[name] = digest(out)
    return res


def tile_child():
    """Body of the child processes of `forced`: every AB_CASES launch under the SGL_NT_TILE of the environment; under 288
    also the launches of NOT_288, which must be refused with the output untouched."""
    import __graft_entry__ as entry
    hl = entry.load_package().lib.load()
    res = all_digests(hl)
    if os.environ.get("SGL_NT_TILE") == "288":
        for name, (b, t, h, hd, hdp) in NOT_288.items():
            for dt in (BF16, F16):
                out = launch_qkv(hl, dt, b, t, h, h * hd, seed=3, hd=hd, hdp=hdp, expect=SGL_ERR_UNSUPPORTED)[0]
                out.check(f"refused {name}", written=False)
                assert bool(torch.isnan(out.got().float()).all()), f"refused {name}: the output was written"
        res["refused"] = sorted(NOT_288)
    print("NT_TILE_DIGESTS " + json.dumps(res))


@pytest.fixture(scope="module")
def forced():
    """{256: digests, 288: digests}: one child process per forced tile."""
    here = os.path.dirname(os.path.abspath(__file__))
    code = (f"import sys; sys.path[:0] = [{os.path.dirname(here)!r}, {here!r}]; "
            f"import test_gemm_nt_288_gpu as t; t.tile_child()")
    res = {}
    for tile in (256, 288):
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


@pytest.mark.parametrize("name", sorted(AB_CASES))
def test_nt288_bitwise_equal_to_256_tile(forced, default, name):
    """Same inputs under SGL_NT_TILE=256 and =288 (and under the default dispatch): identical bits, bf16 and fp16."""
    assert forced[288][name] == forced[256][name], f"{name}: the two tiles disagree"
    assert default[name] == forced[256][name], f"{name}: the default dispatch disagrees with the 256x256 tile"


def test_nt288_forced_tile_refuses_other_shapes(forced):
    """Under SGL_NT_TILE=288: hd = 40, head_dim_pad = 72 and N % 288 != 0 come back SGL_ERR_UNSUPPORTED, nothing written."""
    assert forced[288]["refused"] == sorted(NOT_288)


@pytest.mark.parametrize("name", sorted(NOT_288))
@pytest.mark.parametrize("dtype", [BF16, F16], ids=lambda d: kr.DT_NAME[d])
def test_nt288_default_dispatch_keeps_other_shapes(lib, dtype, name):
    """The default dispatch keeps what the 256x288 tile cannot take on the 256x256 kernel: float64 bound, pad columns +0."""
    b, t, h, hd, hdp = NOT_288[name]
    check_qkv(lib, dtype, b, t, h, h * hd, seed=3, hd=hd, hdp=hdp)


def test_nt288_run_to_run_bitwise(lib):
    a = digest(launch_qkv(lib, BF16, 3, 729, 16, 200, seed=5)[0])
    b = digest(launch_qkv(lib, BF16, 3, 729, 16, 200, seed=5)[0])
    assert a == b


@pytest.mark.parametrize("dtype", [BF16, F16], ids=lambda d: kr.DT_NAME[d])
def test_nt288_nonfinite_contract(lib, dtype):
    """The QKV-scatter cases of tests/nonfinite_util.py (NaN, +inf, -inf at an A, a B and a bias site, first and last element
    of each) at 3 x 729 tokens, 4 heads of 72: rule 1 (no swallowing) and rule 2 (no spreading: every element that does not
    depend on the site keeps the bits of the clean launch), the pad columns +0 whatever the input holds."""
    shape = (3, 729, 4, HD)
    batch, tokens, heads, hd = shape
    D = heads * hd
    inp = {k: v.to("cuda") for k, v in nf.qkv_inputs(dtype, *shape).items()}
    what = f"gemm_nt qkv 288 {kr.DT_NAME[dtype]} {shape}"

    def run(d, poisoned):
        out = run_gemm_nt_qkv(lib, dtype, padded(d["A"], D + 8), padded(d["B"], D + 8), d["bias"], batch, tokens, heads, hd, HDP)
        out.check(what, written=not poisoned)
        got = out.got().view(3, batch, heads, tokens, HDP)
        assert bool((got[..., hd:].contiguous().view(torch.int16) == 0).all()), f"{what}: pad columns must be written as +0"
        return dict(qkv=got[..., :hd])
    nf.drive(what, run, nf.qkv_ref(*shape), inp, nf.qkv_sites(*shape))
