"""SHA-256 digests of what the anti-phase GEMM kernels (csrc/gemm_bf16_v2.hip: the 256x256 and 384x192 NT tiles, the
256x256 TN tile) write for fixed inputs: the record that a refactor of that file moved no output bit.

    python tests/gen_gemm_pp_digests.py        # on an MI355X: writes tests/golden/gemm_pp_parent_digests.json

tests/test_gemm_pp_digests_gpu.py recomputes `digests()` and compares it with that file.  The file is recorded from the
library of the commit BEFORE the change under test, never from the tree that is being checked.

Every launch goes through sgl_op_gemm_nt or sgl_op_gemm_tn_ws with the default dispatch and no environment switch, on
the seeded operands of tests/test_kernel_edges_gpu.py: every leading dimension above the logical width with NaN in the
slack, every output a `Guarded` one.  The digest is taken over the WHOLE guarded allocation, so a write into the guard rows
or into the columns between the width and the leading dimension moves it.  Shapes are the smallest that reach the kernels:

* `nt256/`: M = 2333 (ragged last row tile), (N, K) = (264, 72) and (1160, 200): a last column tile of 8 columns (three
  idle wave columns) and of 136 (a partly filled one), K with a tail.  Epilogues 0, 1, 2, 4, 5, 6 in bf16 and fp16;
  EPI_BIAS_GELU with and without `out`.
* `qkv/`: EPI_QKV at head dims 8, 40, 96 with batch x tokens = 7 x 300, pad columns included.
* `nt384/`: EPI_STORE on (2051, 1152, 1152), (2048, 576, 200), (2304, 384, 64) and EPI_RES_F32 on (2051, 576, 2112).
* `tn256/`: (Mred, N1, N2) = (2048, 512, 512) and (4133, 520, 1152) with a workspace that holds the split slabs (the
  deterministic path), store and accumulate.

The C ABI fixes the output type by the epilogue (16-bit for 0, 1, 3, 4; fp32 for 2, 5, 6), so the fp32-output
instantiations of epilogues 0, 1, 3, 4 (the encoder's bf16x3 mode) are not reachable from here.  Launches that add with
fp32 atomics (TN without a workspace, the bias gradient without a partial-sum buffer) have no fixed summation order and
get no digest.
"""
from __future__ import annotations

import json
import math
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(HERE, "golden", "gemm_pp_parent_digests.json")

BF16, F16 = 1, 3                                          # SGL_DTYPE_*
DT_NAME = {BF16: "bf16", F16: "f16"}
NT256_M, NT256_NK = 2333, [(264, 72), (1160, 200)]
NT256_EPIS = [0, 1, 2, 4, 5, 6]
QKV_CASES = [(7, 300, 12, 8), (7, 300, 4, 40), (7, 300, 3, 96)]          # batch, tokens, heads, head dim
NT384_STORE = [(2051, 1152, 1152), (2048, 576, 200), (2304, 384, 64)]
NT384_RES = [(2051, 576, 2112)]
TN_CASES = [(2048, 512, 512), (4133, 520, 1152)]                         # Mred, N1, N2
TN_WS_BYTES = 64 << 20


def sha(*outs):
    """One digest over the whole allocation (guard rows and slack columns included) of every Guarded output given."""
    import hashlib
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for o in outs:
        h.update(o.ibuf.contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


def nt_case(lib, dtype, M, N, K, epi, seed, with_out=True):
    """The launch of test_kernel_edges_gpu.check_nt_epilogue without its reference."""
    import test_kernel_edges_gpu as te
    g, A, B, bias = te.nt_operands(dtype, M, N, K, seed)
    odt = torch.float32 if epi in (2, 5, 6) else te.tdt_of(dtype)
    out = te.Guarded(M, N, N + 8, odt)
    outs, kw = [out], {}
    if epi == 1:
        out2 = te.Guarded(M, N, N + 16, odt)
        outs.append(out2)
        kw = dict(out2=out2.ptr, ldo2=N + 16)
    if epi == 2:
        kw = dict(res=te.padded(te.randn(g, M, N), N + 8), ldr=N + 8)
    if epi == 4:
        kw = dict(aux=te.padded((te.randn(g, M, N) * 1.5).to(odt), N + 24), ldaux=N + 24)
    if epi == 5:
        kw = dict(pos=te.randn(g, 37, N), pos_rows=37)
    te.ok(te.gemm_nt(lib, dtype, A, K + 8, B, K + 8, M, N, K, epi, out.ptr if with_out else None, N + 8,
                     bias=None if epi == 4 else bias, **kw))
    return sha(*outs)


def qkv_case(lib, dtype, batch, tokens, heads, hd):
    import test_kernel_edges_gpu as te
    g = te.gen(hd + batch)
    tdt = te.tdt_of(dtype)
    D, hdp = heads * hd, te.rup(hd, 16)
    M, N, K = batch * tokens, 3 * D, D
    A = te.padded(te.randn(g, M, K).to(tdt), K + 8)
    B = te.padded((te.randn(g, N, K) / math.sqrt(K)).to(tdt), K + 8)
    bias = te.randn(g, N)
    out = te.Guarded(3 * batch * heads * tokens, hdp, hdp, tdt)
    te.ok(te.gemm_nt(lib, dtype, A, K + 8, B, K + 8, M, N, K, 3, out.ptr, 0, bias=bias, tokens=tokens, heads=heads, hd=hd,
                     hdp=hdp, batch=batch))
    return sha(out)


def tn_case(lib, dtype, Mred, N1, N2, accumulate):
    """The launch of test_kernel_edges_gpu.check_tn with a workspace, without its reference."""
    import test_kernel_edges_gpu as te
    g = te.gen(Mred + N1)
    tdt = te.tdt_of(dtype)
    lda, ldb, ldo = te.rup(N1, 8) + 8, te.rup(N2, 8) + 8, te.rup(N2, 4) + 4
    A = te.padded(te.randn(g, Mred, N1).to(tdt), lda)
    B = te.padded(te.randn(g, Mred, N2).to(tdt), ldb)
    prior = te.randn(g, N1, N2) * 3 if accumulate else None
    out = te.Guarded(N1, N2, ldo, torch.float32, prior=prior)
    ws = torch.empty(TN_WS_BYTES, device=te.DEV, dtype=torch.uint8)
    te.ok(lib.sgl_op_gemm_tn_ws(dtype, te.P(A), lda, te.P(B), ldb, Mred, N1, N2, 1, out.ptr, ldo, accumulate, te.P(ws),
                                TN_WS_BYTES, te.stream()))
    return sha(out)


def digests(lib) -> dict:
    """case name -> SHA-256, for every case of the file's docstring.  `lib` is the loaded C-ABI library."""
    d = {}
    for dtype in (BF16, F16):
        dn = DT_NAME[dtype]
        for N, K in NT256_NK:
            for epi in NT256_EPIS:
                d[f"nt256/{dn}/N{N}_K{K}/epi{epi}"] = nt_case(lib, dtype, NT256_M, N, K, epi, seed=N + epi)
            d[f"nt256/{dn}/N{N}_K{K}/epi1_without_out"] = nt_case(lib, dtype, NT256_M, N, K, 1, seed=N + 1, with_out=False)
        for batch, tokens, heads, hd in QKV_CASES:
            d[f"qkv/{dn}/b{batch}_t{tokens}_h{heads}_d{hd}"] = qkv_case(lib, dtype, batch, tokens, heads, hd)
        for M, N, K in NT384_STORE:
            d[f"nt384/{dn}/M{M}_N{N}_K{K}/epi0"] = nt_case(lib, dtype, M, N, K, 0, seed=M + K)
        for M, N, K in NT384_RES:
            d[f"nt384/{dn}/M{M}_N{N}_K{K}/epi2"] = nt_case(lib, dtype, M, N, K, 2, seed=M + K)
        for Mred, N1, N2 in TN_CASES:
            for acc in (0, 1):
                d[f"tn256/{dn}/Mred{Mred}_{N1}x{N2}/{'accumulate' if acc else 'store'}"] = tn_case(lib, dtype, Mred, N1, N2, acc)
    return d


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    import __graft_entry__ as g
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    d = digests(g.load_package().lib.load())
    with open(out, "w") as f:
        json.dump(d, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {out}: {len(d)} digests")


if __name__ == "__main__":
    main()
