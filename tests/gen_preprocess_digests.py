"""SHA-256 digests of what the input pipeline (csrc/preprocess.hip, csrc/video_tail.hip) writes for fixed inputs, through
the C ABI: the record that a refactor of those files moved no output bit.

    python tests/gen_preprocess_digests.py        # on an MI355X: writes tests/golden/preprocess_parent_digests.json

tests/test_preprocess_digests_gpu.py recomputes `digests()` and compares it with that file.  The file is recorded from
the library of the commit BEFORE the change under test, never from the tree that is being checked.

Inputs come from an integer formula on the CPU, no RNG library, so they cannot drift: v(i) = (i * 2654435761 + seed)
mod 2^32, its top 8 bits for uint8 sources, v / 2^32 in float64 cast to fp32 for float sources and for output gradients;
the seed is the CRC-32 of the case's name.  Every output buffer is pre-filled with 0x5A bytes, so an element that a
kernel leaves unwritten is part of the digest too.
"""
from __future__ import annotations

import hashlib
import json
import os
import sys
import zlib

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(HERE, "golden", "preprocess_parent_digests.json")
DEV = "cuda"

# (Hs, Ws) -> S of the plain forward; the S = 45 case drops the pixels past the last whole 14-pixel patch
FWD_GEOMS = [((97, 131), 42), ((30, 30), 42), ((42, 97), 42), ((42, 42), 42)]
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
NCHW = (1, 3, 0)                                         # (P, Kp, patch_major) as preprocess.py passes them
PATCH = (14, 640, 1)                                     # 3 * 14 * 14 = 588 live columns, 52 pad columns
PATCH_SMALL = (4, 64, 1)                                 # for S < 14 (the `coverage` views, S = 12): 48 live, 16 pad
MIX = ([2, 2, 0], 0.3)                                   # not a permutation
AUG_RECORDS = [
    dict(flip=False, cos=1.0, sin=0.0, brightness=1.0, contrast=1.0, saturation=1.0, hue=0.0, order=None),
    dict(flip=True, cos=1.0, sin=0.0, brightness=1.0, contrast=1.0, saturation=1.0, hue=0.0, order=None),
    dict(flip=False, cos=0.9961946980917455, sin=0.08715574274765817, brightness=1.07, contrast=0.93, saturation=1.06,
         hue=0.04, order=[0, 2, 1, 3]),                  # 5 degrees; contrast third
    dict(flip=True, cos=1.0, sin=0.0, brightness=0.94, contrast=1.0, saturation=0.92, hue=-0.03, order=[2, 0, 3, 3]),
]
VIEW_CASES = ["orientation", "scale_copy_turn_and_flip", "coverage", "chunk_V65", "app"]


def values(n, name):
    """v(i), i < n, as int64 in [0, 2^32)."""
    seed = zlib.crc32(name.encode())
    return (torch.arange(n, dtype=torch.int64) * 2654435761 + seed) & 0xFFFFFFFF


def floats(shape, name):
    n = 1
    for s in shape:
        n *= s
    return (values(n, name).double() / 2.0 ** 32).float().view(*shape)


def source(B, Hs, Ws, u8, name):
    """uint8 NHWC bytes or float NCHW in [0, 1) on the device."""
    if u8:
        return (values(B * Hs * Ws * 3, name) >> 24).to(torch.uint8).view(B, Hs, Ws, 3).to(DEV)
    return floats((B, 3, Hs, Ws), name).to(DEV)


def blank(shape, dtype):
    return torch.empty(shape, device=DEV, dtype=dtype).view(torch.uint8).fill_(0x5A).view(dtype).view(*shape)


def sha(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def out_rows(n, S, layout, dtype):
    P, Kp, patch_major = layout
    return blank((n * (S // P) ** 2, Kp) if patch_major else (n, 3, S, S), dtype)


def view_table(lib_mod, views):
    tab = (lib_mod.SglView * len(views))()
    for n, (b, box, turns, keep, flip) in enumerate(views):
        tab[n] = lib_mod.SglView(int(b), *(int(t) for t in box), int(turns), int(keep), int(flip))
    return tab


def digests(pkg) -> dict:
    """case name -> SHA-256 of the output bytes, for every case of the file's docstring."""
    import views_bwd_ref as vb
    import views_ref as vr
    from test_preprocess_bwd_gpu import BRANCHES
    import preprocess_bwd_ref as pb

    L, pp = pkg.lib, pkg.preprocess
    lib = L.load()
    out = {}

    # ---- forward, plain ------------------------------------------------------------------------------------------
    def forward(name, Hs, Ws, S, u8, dt, layout, mix):
        B = 3
        src = source(B, Hs, Ws, u8, name)
        dst = out_rows(B, S, layout, DTYPES[dt])
        idx = None if mix is None else torch.tensor(mix[0], dtype=torch.int32, device=DEV)
        L.call("sgl_op_preprocess", DEV, src.data_ptr(), int(u8), B, Hs, Ws, dst.data_ptr(), L.dtype_code(DTYPES[dt]), S,
               *layout, 0.5, 0.5, L.ptr(idx), 1.0 if mix is None else mix[1])
        out[name] = sha(dst)

    for (Hs, Ws), S in FWD_GEOMS:
        for u8 in (True, False):
            for dt in DTYPES:
                for lname, layout in (("nchw", NCHW), ("patch", PATCH)):
                    for mix in (None, MIX):
                        name = f"fwd/{Hs}x{Ws}to{S}/{'u8' if u8 else 'f32'}/{dt}/{lname}/{'mix' if mix else 'nomix'}"
                        forward(name, Hs, Ws, S, u8, dt, layout, mix)
    for u8 in (True, False):
        for mix in (None, MIX):
            forward(f"fwd/97x131to45/{'u8' if u8 else 'f32'}/bf16/patch_dropped/{'mix' if mix else 'nomix'}", 97, 131, 45, u8,
                    "bf16", PATCH, mix)

    # ---- augmentation --------------------------------------------------------------------------------------------
    tab = pp.augment_table(AUG_RECORDS, DEV)
    for S in (42, 45):
        for u8 in (True, False):
            for lname, layout, dt in (("nchw", NCHW, "f32"), ("patch", PATCH, "bf16")):
                name = f"aug/59x101to{S}/{'u8' if u8 else 'f32'}/{dt}/{lname}"
                B, Hs, Ws = 4, 59, 101
                src = source(B, Hs, Ws, u8, name)
                dst = out_rows(B, S, layout, DTYPES[dt])
                gm = blank((B,), torch.float32)
                L.call("sgl_op_preprocess_aug", DEV, src.data_ptr(), int(u8), B, Hs, Ws, dst.data_ptr(),
                       L.dtype_code(DTYPES[dt]), S, *layout, 0.5, 0.5, tab.data_ptr(), gm.data_ptr())
                out[name] = sha(dst)
                out[name + "/grey_mean"] = sha(gm)

    # ---- views, forward and backward -----------------------------------------------------------------------------
    cases = vb.cases(pp)
    for case in VIEW_CASES:
        B, Hs, Ws, S, views = cases[case]
        views = [vr.as_tuple(v) for v in views]
        V, vt = len(views), view_table(L, views)
        for u8, dt, lname, layout in ((True, "bf16", "patch", PATCH if S >= 14 else PATCH_SMALL), (False, "f32", "nchw", NCHW)):
            name = f"views/{case}/{'u8' if u8 else 'f32'}/{dt}/{lname}"
            src = source(B, Hs, Ws, u8, name)
            dst = out_rows(V, S, layout, DTYPES[dt])
            L.call("sgl_op_preprocess_views", DEV, src.data_ptr(), int(u8), B, Hs, Ws, vt, V, dst.data_ptr(),
                   L.dtype_code(DTYPES[dt]), S, *layout, 0.5, 0.5, None, 0)
            out[name] = sha(dst)
        name = f"views_bwd/{case}"
        G = floats((V, 3, S, S), name).to(DEV)
        d_src = blank((B, 3, Hs, Ws), torch.float32)
        nbytes = lib.sgl_op_preprocess_views_bwd_scratch_bytes(vt, V, S)
        scratch = blank((nbytes,), torch.uint8) if nbytes else None
        L.call("sgl_op_preprocess_views_bwd", DEV, G.data_ptr(), B, Hs, Ws, vt, V, S, 0.5, d_src.data_ptr(), L.ptr(scratch),
               nbytes)
        out[name] = sha(d_src)

    # ---- plain backward ------------------------------------------------------------------------------------------
    for branch, (Hs, Ws), S in BRANCHES:
        for n, (mix, lam) in enumerate(pb.MIXES):
            name = f"bwd/{branch}/{'nomix' if mix is None else f'mix_lam{lam}'}"
            B = 3
            G = floats((B, 3, S, S), name).to(DEV)
            idx = None if mix is None else torch.tensor(mix, dtype=torch.int32, device=DEV)
            d_src = blank((B, 3, Hs, Ws), torch.float32)
            nbytes = lib.sgl_op_preprocess_bwd_scratch_bytes(B, Hs, Ws, S)
            scratch = blank((nbytes,), torch.uint8) if nbytes else None
            L.call("sgl_op_preprocess_bwd", DEV, G.data_ptr(), B, Hs, Ws, S, 0.25, L.ptr(idx), lam, d_src.data_ptr(),
                   L.ptr(scratch), nbytes)
            out[name] = sha(d_src)

    # ---- video tail ----------------------------------------------------------------------------------------------
    B, T, D = 2, 3, 300
    f = (floats((B * T, D), "video_tail/f") - 0.5).to(DEV)
    g = (floats((B, D), "video_tail/g") - 0.5).to(DEV)
    mean, inv, df = blank((B, D), torch.float32), blank((B * T,), torch.float32), blank((B * T, D), torch.float32)
    L.call("sgl_op_l2norm_tmean_fwd", DEV, f.data_ptr(), mean.data_ptr(), inv.data_ptr(), B, T, D)
    L.call("sgl_op_l2norm_tmean_bwd", DEV, f.data_ptr(), inv.data_ptr(), g.data_ptr(), df.data_ptr(), B, T, D)
    out["video_tail/fwd/out"], out["video_tail/fwd/inv_norm"], out["video_tail/bwd/df"] = sha(mean), sha(inv), sha(df)
    return out


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    import __graft_entry__ as g
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    d = digests(g.load_package())
    with open(out, "w") as f:
        json.dump(d, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {out}: {len(d)} digests")


if __name__ == "__main__":
    main()
