"""Return codes and SHA-256 digests of what the attention entry points (sgl_op_attn_fwd / _bwd, sgl_op_attn_probs,
sgl_op_pool_attn_fwd / _bwd) write for fixed inputs: the record that the consolidation of their host front (one shape
contract, one dispatcher, one head addressing: csrc/attention.hip.h) moved no output bit and no refusal.

    SGL_LIB_PATH=<parent build>/libsiglip_hip.so python tests/gen_attn_digests.py   # on an MI355X

writes tests/golden/attn_parent_digests.json = {case: {"rc": [status codes], "sha": digest}}.  The file is recorded from
the library of the commit BEFORE the change under test (SGL_LIB_PATH names it), never from the tree that is being checked;
tests/test_attn_digests_gpu.py recomputes `digests()` on the tree's own library and compares.

Every output is a `Guarded` one (tests/attn_util.py) and the digest covers its WHOLE allocation, guard rows included.  No
attention path uses atomics, so every case is deterministic.  The cases are the smallest that reach every route:

* `fwdbwd/`: all four dtypes x {token, head} layout at (B, H, N, dh) = (1,3,65,8), (2,2,130,72), (1,2,300,96), (1,9,33,64):
  DP 16, 80, 96 and 64, one and several key tiles, a ragged last tile, B*H below and above the 8 XCDs.  O, lse and dqkv.
* `probs/`: all four dtypes x {FULL, HEAD_MEAN} at (2,3,130,72) and (1,2,33,8), on the lse of sgl_op_attn_fwd itself.
* `pool/`: forward and backward (on the forward's own probabilities) in bf16, fp16 and fp32 at (2,3,130,72).
* `refuse/`: one refused argument set per rule of the shape contract, per dtype route that has the rule, plus the 16-bit
  alignment refusal (q two bytes off).  Refused calls must not launch: the digest is that of untouched outputs, and the
  test asserts it separately.  A refused call never reads its operands, so the huge-extent cases pass small buffers.
"""
from __future__ import annotations

import hashlib
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(HERE, "golden", "attn_parent_digests.json")

F32, BF16, BF16X3, F16 = 0, 1, 2, 3                       # SGL_DTYPE_*
DT_NAME = {F32: "f32", BF16: "bf16", BF16X3: "bf16x3", F16: "f16"}
FWDBWD_SHAPES = [(1, 3, 65, 8), (2, 2, 130, 72), (1, 2, 300, 96), (1, 9, 33, 64)]
PROBS_SHAPES = [(2, 3, 130, 72), (1, 2, 33, 8)]
POOL_SHAPE = (2, 3, 130, 72)

# refused (dtype route, pass) argument sets: B, H, N, dh, DP, ld, and whether q sits two bytes off.  Base: 1, 2, 40, 16, 16.
BIG_EXTENT_N = 1 << 26          # 16-bit: N * row bytes >= 2^31 from 32-byte rows (probs, DP = 16) up
BIG_OUT_N = 1 << 21             # 16-bit, head-major, H = 64, dh = 8: N * DP * 2 < 2^31 <= N * H * dh * 2
GRID_N_MFMA = 46341 * 128       # probs: ceil(N / 128)^2 >= 2^31
GRID_N_STRICT = 741456          # probs: ceil(N / 4) * ceil(N / 64) >= 2^31
REFUSE_FWDBWD = {
    "lo": [("dh_mod8", dict(dh=12)), ("dp_not_roundup16", dict(dh=8, DP=32)), ("dp_not_instantiated", dict(dh=104, DP=112)),
           ("ld_negative", dict(ld=-8)), ("ld_mod8", dict(ld=100)), ("ld_below_heads", dict(ld=24)),
           ("qkv_extent_2g", dict(N=BIG_EXTENT_N)), ("out_extent_2g", dict(H=64, N=BIG_OUT_N, dh=8, ld=0)),
           ("q_misaligned", dict(off=2))],
    "bf16x3": [("dh_mod8", dict(dh=12, DP=12)), ("dh_above_96", dict(dh=104, DP=104)), ("dp_below_dh", dict(dh=16, DP=8)),
               ("dp_mod4", dict(dh=8, DP=10)), ("ld_negative", dict(ld=-8)), ("ld_mod4", dict(ld=98)),
               ("ld_below_heads", dict(ld=24)), ("n_negative", dict(N=-1))],
    "f32": [("dh_above_128", dict(dh=136, DP=144)), ("lds_fwd_and_bwd", dict(N=10113)),
            ("lds_bwd_only", dict(N=4993, fwd=False))],
}
REFUSE_PROBS = {
    "lo": [("dh_mod8", dict(dh=12)), ("dp_not_roundup16", dict(dh=8, DP=32)), ("dp_above_96", dict(dh=104, DP=112)),
           ("qk_extent_2g", dict(N=BIG_EXTENT_N)), ("grid", dict(N=GRID_N_MFMA)), ("q_misaligned", dict(off=2)),
           ("dh_above_dp", dict(dh=32, DP=16)), ("n_zero", dict(N=0)), ("mode_unknown", dict(mode=2))],
    "bf16x3": [("dh_mod8", dict(dh=12, DP=12)), ("dh_above_96", dict(dh=104, DP=104)), ("dp_mod4", dict(dh=8, DP=10)),
               ("grid", dict(N=GRID_N_MFMA))],
    "f32": [("dh_above_128", dict(dh=136, DP=144)), ("grid", dict(N=GRID_N_STRICT))],
}
ROUTE_DTYPES = {"lo": (BF16, F16), "bf16x3": (BF16X3,), "f32": (F32,)}


def sha(*outs):
    """One digest over the whole allocation (guard rows and slack columns included) of every Guarded output given."""
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for o in outs:
        h.update(o.ibuf.contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


def fwdbwd_case(lib, dtype, layout, B, H, N, dh):
    import attn_util as au
    import kernel_ref as kr
    q, k, v, do = kr.attn_inputs("gauss", B, H, N, dh, au.tdt_of(dtype), seed=N + dh)
    st_f, st_b, out, lse, dqkv = au.launch_attention(lib, dtype, layout, q, k, v, do)
    return {"rc": [st_f, st_b], "sha": sha(out, lse, dqkv)}


def probs_case(lib, dtype, B, H, N, dh):
    """FULL and HEAD_MEAN maps from head-major q, k and the lse of sgl_op_attn_fwd on the same operands."""
    import attn_util as au
    import kernel_ref as kr
    tdt = au.tdt_of(dtype)
    DP, D = au.rup(dh, 16), H * dh
    q, k, v, _ = kr.attn_inputs("gauss", B, H, N, dh, tdt, seed=N + dh)
    qkv = torch.zeros(3, B, H, N, DP, device=au.DEV, dtype=tdt)
    qkv[..., :dh] = torch.stack((q, k, v)).to(au.DEV)
    out = au.Guarded(B * N, D, D, tdt)
    lse = au.Guarded(1, B * H * N, B * H * N, torch.float32)
    st_f = lib.sgl_op_attn_fwd(dtype, au.P(qkv[0]), au.P(qkv[1]), au.P(qkv[2]), out.ptr, lse.ptr, B, H, N, dh, DP, 0,
                               au.stream())
    res = {}
    for mode, name in ((0, "full"), (1, "head_mean")):
        pm = au.Guarded(B * (1 if mode else H) * N, N, N, torch.float32)
        st = lib.sgl_op_attn_probs(dtype, au.P(qkv[0]), au.P(qkv[1]), lse.ptr, pm.ptr, B, H, N, dh, DP, mode, au.stream())
        res[name] = {"rc": [st_f, st], "sha": sha(pm)}
    return res


def pool_case(lib, dtype, B, H, N, dh):
    import attn_util as au
    import kernel_ref as kr
    tdt = au.tdt_of(dtype)
    DP = au.rup(dh, 16)
    q, K, V, do = (t.to(au.DEV) for t in kr.pool_inputs("gauss", B, H, N, dh, DP, tdt, seed=B + H))
    out, probs = au.Guarded(B, H * dh, H * dh, tdt), au.Guarded(B * H, N, N, torch.float32)
    st_f = lib.sgl_op_pool_attn_fwd(dtype, au.P(q), au.P(K), au.P(V), out.ptr, probs.ptr, B, H, N, dh, DP, au.stream())
    dkv, dq = au.Guarded(B * N, 2 * H * dh, 2 * H * dh, tdt), au.Guarded(B, H * dh, H * dh, torch.float32)
    st_b = lib.sgl_op_pool_attn_bwd(dtype, au.P(q), au.P(K), au.P(V), probs.ptr, au.P(do), dkv.ptr, dq.ptr, B, H, N, dh, DP,
                                    au.stream())
    return {"rc": [st_f, st_b], "sha": sha(out, probs, dkv, dq)}


def refusal_outputs(n):
    """`n` small guarded outputs and the digest they have while nothing has written them."""
    import attn_util as au
    outs = [au.Guarded(8, 64, 64, torch.float32) for _ in range(n)]
    return outs, sha(*outs)


def refusal_case(lib, dtype, probs, B=1, H=2, N=40, dh=16, DP=None, ld=None, off=0, mode=0, fwd=True):
    """One refused call (forward and backward, or probs) on small zeroed operands; -> (entry, digest of untouched outputs)."""
    import attn_util as au
    DP = au.rup(dh, 16) if DP is None else DP
    ld = (0 if probs else 3 * H * dh + 8) if ld is None else ld
    src = torch.zeros(1 << 16, device=au.DEV, dtype=torch.uint8)
    lse_in = torch.zeros(1 << 12, device=au.DEV)
    p = au.P(src)
    s = au.stream()
    if probs:
        outs, clean = refusal_outputs(1)
        rc = [lib.sgl_op_attn_probs(dtype, p + off, p + 4096, au.P(lse_in), outs[0].ptr, B, H, N, dh, DP, mode, s)]
    else:
        outs, clean = refusal_outputs(4)
        o, lse, dqkv, delta = (g.ptr for g in outs)
        rc = [lib.sgl_op_attn_fwd(dtype, p + off, p + 4096, p + 8192, o, lse, B, H, N, dh, DP, ld, s)] if fwd else []
        rc.append(lib.sgl_op_attn_bwd(dtype, p + off, p + 4096, p + 8192, p + 12288, p + 16384, au.P(lse_in), dqkv, delta,
                                      B, H, N, dh, DP, ld, s))
    return {"rc": rc, "sha": sha(*outs)}, clean


def digests(lib, clean: dict | None = None) -> dict:
    """case name -> {"rc", "sha"} for every case of the file's docstring.  `lib` is the loaded C-ABI library.  `clean`
    (optional) receives, per refusal case, the digest its outputs had before the call."""
    d = {}
    for dtype, dn in DT_NAME.items():
        for layout in ("token", "head"):
            for B, H, N, dh in FWDBWD_SHAPES:
                d[f"fwdbwd/{dn}/{layout}/B{B}_H{H}_N{N}_dh{dh}"] = fwdbwd_case(lib, dtype, layout, B, H, N, dh)
        for B, H, N, dh in PROBS_SHAPES:
            for mode, e in probs_case(lib, dtype, B, H, N, dh).items():
                d[f"probs/{dn}/{mode}/B{B}_H{H}_N{N}_dh{dh}"] = e
        if dtype != BF16X3:
            B, H, N, dh = POOL_SHAPE
            d[f"pool/{dn}/B{B}_H{H}_N{N}_dh{dh}"] = pool_case(lib, dtype, B, H, N, dh)
    for table, probs in ((REFUSE_FWDBWD, False), (REFUSE_PROBS, True)):
        for route, cases in table.items():
            for dtype in ROUTE_DTYPES[route]:
                for rule, kw in cases:
                    name = f"refuse/{'probs' if probs else 'fwdbwd'}/{DT_NAME[dtype]}/{rule}"
                    d[name], c = refusal_case(lib, dtype, probs, **kw)
                    if clean is not None:
                        clean[name] = c
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
    print(f"wrote {out}: {len(d)} cases")


if __name__ == "__main__":
    main()
