"""What sgl_adamw_bind_shadows (host only: no GPU is touched) binds for every master tensor of the encoder: the record
that a change to the shadow placement table of csrc/encoder.hip moved no copy.

    python tests/gen_shadow_binding.py            # writes tests/golden/shadow_binding_parent.json

tests/test_shadow_binding_host.py recomputes `records()` and compares every field with that file.  The file is recorded
from the library of the commit BEFORE the change under test (SGL_LIB_PATH names that library), never from the tree that
is being checked.

Configs `tiny` and `hostile`, with and without the pooling head, every compute dtype sgl_create accepts.  The sgl_weights
struct holds distinct fake non-zero addresses (nothing is dereferenced), the host table names each of them once, and every
aux entry is pre-filled with PREFILL so that a field the function leaves alone shows as left alone.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(HERE, "golden", "shadow_binding_parent.json")

CONFIGS = ["tiny", "hostile"]
MODES = {"fp32": 0, "bf16": 1, "bf16x3": 2, "fp16": 3, "mxfp8": 5}        # SGL_DTYPE_*
GLOBAL_FIELDS = ["patch_w", "patch_b", "pos", "post_ln_w", "post_ln_b"]
MASTER0, MASTER_STEP = 0x10000000, 0x100000                              # fake fp32 masters
SHADOW = 0x7F0000000000                                                  # fake arena base
PREFILL = -7
INT_FIELDS = ["ld", "ld_t", "rows", "cols", "row0", "dtype", "group", "reserved"]
PTR_FIELDS = ["dst", "dst_t", "dst_f32", "ema"]
EMA = 0x5A5A0000                                                         # must survive the call


def case_name(cfg, head, mode):
    return f"{cfg}/{'head' if head else 'nohead'}/{mode}"


def one(pkg, lib, cfg_name, use_head, mode):
    L = pkg.lib
    cfg = dataclasses.replace(pkg.get_config(cfg_name), vision_use_head=bool(use_head))
    c = L.SglConfig(cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers, cfg.num_attention_heads,
                    cfg.patch_size, cfg.native_grid, cfg.layer_norm_eps, MODES[mode], int(use_head))
    ctx = lib.sgl_create(C.byref(c))
    assert ctx, f"sgl_create({cfg_name}, {mode}) returned NULL"
    try:
        nl = cfg.num_hidden_layers
        layers = (L.SglLayerPtrs * nl)()
        w = L.SglWeights()
        w.layers = C.cast(layers, C.POINTER(L.SglLayerPtrs))
        names, addr = [], MASTER0
        for f in GLOBAL_FIELDS + L.HEAD_FIELDS:
            setattr(w, f, addr)
            names.append(f)
            addr += MASTER_STEP
        for l in range(nl):
            for f in L.LAYER_FIELDS:
                setattr(layers[l], f, addr)
                names.append(f"layers.{l}.{f}")
                addr += MASTER_STEP
        n = len(names)
        table = (L.SglAdamwTensor * n)()
        aux = (L.SglAdamwAux * n)()
        for i in range(n):
            table[i].p = MASTER0 + i * MASTER_STEP
            for f in INT_FIELDS:
                setattr(aux[i], f, PREFILL)
            aux[i].ema = EMA
        ret = lib.sgl_adamw_bind_shadows(ctx, C.byref(w), SHADOW, table, aux, n)
        masters = {}
        for i, name in enumerate(names):
            a = aux[i]
            rec = {f: (None if not getattr(a, f) else getattr(a, f) - SHADOW) for f in PTR_FIELDS[:3]}
            rec.update({f: getattr(a, f) for f in INT_FIELDS})
            rec["ema"] = a.ema
            untouched = all(rec[f] is None for f in PTR_FIELDS[:3]) and all(rec[f] == PREFILL for f in INT_FIELDS) \
                and a.ema == EMA
            masters[name] = None if untouched else rec       # None: the entry is exactly as it was before the call
        return {"return": ret, "masters": masters}
    finally:
        lib.sgl_destroy(ctx)


def records(pkg) -> dict:
    lib = pkg.lib.load()
    return {case_name(cfg, head, mode): one(pkg, lib, cfg, head, mode)
            for cfg in CONFIGS for head in (1, 0) for mode in MODES}


def main():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    r = records(g.load_package())
    with open(out, "w") as f:
        json.dump(r, f, indent=0, sort_keys=True, separators=(",", ":"))
        f.write("\n")
    print(f"wrote {out}: {len(r)} cases, {sum(len(v['masters']) for v in r.values())} masters")


if __name__ == "__main__":
    main()
