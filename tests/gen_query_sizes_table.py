"""Dump sgl_query_sizes over a sweep of (config, mode, policy, train, shape) as JSON: the table
tests/test_input_grad_host.py holds the library to (tests/golden/pixgrad/query_sizes_parent.json).

The table was first written by the library built from the commit BEFORE the input-gradient entry points were added
(they take a scratch argument of their own so that nothing here moves).  It was written again when sgl_query_sizes
learnt the pooling head's token limit (csrc/kernels.h, pool_attn_max_tokens): 317 of the 2166 entries, every shape with
more tokens per image than the head takes (so400m at 384 x 1152 and 771 x 398, large at 384 x 1152 for training), went
from sizes for a call that would have failed to [-1, 0, 0, 0]; no other entry moved.  To regenerate it from an earlier
commit, build that commit's library and point SGL_LIB_PATH at it:

    SGL_LIB_PATH=<parent checkout>/…/libsiglip_hip.so python tests/gen_query_sizes_table.py

Needs no GPU: sgl_query_sizes is host arithmetic.
"""
from __future__ import annotations

import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(HERE, "golden", "pixgrad", "query_sizes_parent.json")

CONFIGS = ["tiny", "hostile", "so400m-1layer", "base-1layer", "so400m-patch14-384", "large-patch16-384"]
MODES = {"fp32": 0, "bf16": 1, "bf16x3": 2, "fp16": 3, "mxfp8": 5}
BATCHES = [1, 2, 5, 128]


def shapes(cfg):
    P, S = cfg.patch_size, cfg.image_size
    return [(P, P), (S, S), (S + P - 1, S + 1), (2 * S + 3, S + P), (S, 3 * S)]


def sweep(pkg, lib):
    """{key: [status, shadow_bytes, saved_bytes, ws_bytes]}, key = config/mode/policy/train/B/H/W."""
    table = {}
    for name in CONFIGS:
        cfg = pkg.get_config(name)
        for mode, code in MODES.items():
            for rc in (0, 1):
                c = pkg.lib.SglConfig(cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers,
                                      cfg.num_attention_heads, cfg.patch_size, cfg.native_grid, cfg.layer_norm_eps, code, 1)
                ctx = lib.sgl_create_ex(C.byref(c), rc)
                if not ctx:
                    table[f"{name}/{mode}/{rc}"] = None     # refused (mxfp8 with a recompute policy)
                    continue
                try:
                    for train in (0, 1):
                        for B in BATCHES:
                            for H, W in shapes(cfg):
                                a, b, d = C.c_size_t(), C.c_size_t(), C.c_size_t()
                                st = lib.sgl_query_sizes(ctx, B, H, W, train, C.byref(a), C.byref(b), C.byref(d))
                                table[f"{name}/{mode}/{rc}/{train}/{B}/{H}/{W}"] = \
                                    [st] + ([a.value, b.value, d.value] if st == 0 else [0, 0, 0])
                finally:
                    lib.sgl_destroy(ctx)
    return table


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    pkg = g.load_package()
    lib = C.CDLL(pkg.lib.LIB_PATH)      # plain handle: an older library lacks symbols today's header declares
    lib.sgl_create_ex.restype = C.c_void_p
    lib.sgl_create_ex.argtypes = [C.POINTER(pkg.lib.SglConfig), C.c_int]
    lib.sgl_destroy.argtypes = [C.c_void_p]
    psz = C.POINTER(C.c_size_t)
    lib.sgl_query_sizes.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, psz, psz, psz]
    t = sweep(pkg, lib)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(t, f, indent=0, sort_keys=True)
    print(f"wrote {OUT}: {len(t)} entries from {pkg.lib.LIB_PATH}")
