"""SHA-256 digests of what the parameter-side passes write for fixed inputs: gradient norm, EMA, AdamW (linear and tiled,
with weight shadows), the weight re-cast (csrc/optimizer.hip, csrc/elementwise.hip cast_job_kernel / split3, and the
shadow placement of csrc/encoder.hip): the record that a refactor of that code moved no output bit.

    python tests/gen_param_pass_digests.py        # on an MI355X: writes tests/golden/param_pass_parent_digests.json

tests/test_param_pass_digests_gpu.py recomputes `digests()` and compares it with that file.  The file is recorded from
the library of the commit BEFORE the change under test, never from the tree that is being checked.

Inputs come from the integer formula of tests/gen_preprocess_digests.py (no RNG library).  Every tensor a kernel may write
is cut from a pool pre-filled with 0x5A bytes and the WHOLE pool is digested, so a write between two tensors, into a
shadow's padding or past an end is part of the digest.  Four families:

* `table/`: the mixed table of tests/test_kernel_edges_aux_gpu.py (sizes 1, 3, 4096, 4097, 12289, tensors 4 bytes off
  alignment, one entry without a gradient) through sgl_op_grad_norm, sgl_op_grad_norm_scaled, sgl_op_ema, sgl_op_adamw and
  sgl_op_adamw_ex (dst_f32 and EMA on aligned and unaligned entries, two hyper-parameter groups);
* `tiled/`: the 64x64-tile path of sgl_op_adamw_ex on TILED_MATS, destination only or both copies, leading dimensions
  padded beyond the columns, bf16 / fp16 / fp32 shadows, with and without EMA, step 1 and step 1000;
* `model/`: `tiny` and `hostile` in every compute mode: the whole shadow arena after each of two FusedAdamW steps with
  attach_encoder and attach_ema, and the arena of a twin model after a fresh re-cast of the same parameters (mxfp8, which
  does not train: the re-cast arena only);
* `cast_job/`, `split3/`: sgl_op_cast_job and sgl_op_split3 on the shapes of tests/test_kernel_edges_internal_gpu.py.
"""
from __future__ import annotations

import ctypes as C
import json
import os
import sys

import torch

from gen_preprocess_digests import DEV, floats, sha

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(HERE, "golden", "param_pass_parent_digests.json")

F32, BF16, F16 = 0, 1, 3                                  # SGL_DTYPE_*
TDT = {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16}
DT_NAME = {F32: "f32", BF16: "bf16", F16: "f16"}
B1, B2, EPS = 0.9, 0.999, 1e-8
MAX_NORMS = [0.0, 0.37, 1e6]
# (rows, cols, row0, which of p/g/m/v sit 4 bytes off): one whole tile; partial tiles; columns not a multiple of 4 (the
# scalar path); several tiles each way; rows [48, 144) shadowed only (the pooling head's in_proj_w).  The (65, 60)
# gradient is 4 bytes off: the scalar path at a column count that IS a multiple of 4.
TILED_MATS = [(64, 64, 0, ""), (65, 60, 0, "g"), (70, 62, 0, ""), (144, 200, 0, ""), (3 * 48, 48, 48, "")]
MODEL_CONFIGS = ["tiny", "hostile"]
TRAIN_MODES = ["fp32", "bf16", "bf16x3", "fp16"]


def rup(x, m):
    return (x + m - 1) // m * m


class Pool:
    """One buffer of 0x5A bytes from which tensors are cut at 256-byte boundaries (+ `off` bytes), 64 bytes apart at least."""

    def __init__(self, nbytes):
        self.buf = torch.empty(nbytes, dtype=torch.uint8, device=DEV).fill_(0x5A)
        self.at = 0

    def take(self, n, dtype=torch.float32, off=0, init=None):
        es = torch.empty(0, dtype=dtype).element_size()
        start = rup(self.at, 256) + off
        self.at = start + n * es + 64
        assert self.at <= self.buf.numel(), "pool too small"
        t = self.buf[start:start + n * es].view(dtype)
        if init is not None:
            t.copy_(init.reshape(-1))
        return t


def state(pool, n, name, off=""):
    """p, g, m, v of n elements in the pool, values by formula; `off` names the ones 4 bytes off 16-byte alignment."""
    vals = dict(p=floats((n,), name + "/p") - 0.5, g=(floats((n,), name + "/g") - 0.5) * 0.02,
                m=(floats((n,), name + "/m") - 0.5) * 0.02, v=floats((n,), name + "/v") * 1e-4)
    return {k: pool.take(n, off=4 if k in off else 0, init=vals[k]) for k in "pgmv"}


_KEEP = []                                               # device tables stay alive until their family is done


def upload(structs):
    _KEEP.append(torch.frombuffer(bytearray(bytes(structs)), dtype=torch.uint8).to(DEV))
    return _KEEP[-1]


def plan(lib, numel):
    arr = (C.c_uint64 * len(numel))(*numel)
    nb = lib.sgl_adamw_plan(arr, len(numel), None, 0)
    bm = (C.c_int32 * (2 * nb))()
    assert lib.sgl_adamw_plan(arr, len(numel), bm, nb) == nb
    return torch.tensor(list(bm), dtype=torch.int32, device=DEV), nb


def mixed_table(L, lib, name):
    from test_kernel_edges_aux_gpu import ADAMW_ENTRIES
    pool = Pool(sum(n for n, _, _ in ADAMW_ENTRIES) * 4 * 6 + 4096 * len(ADAMW_ENTRIES))
    table = (L.SglAdamwTensor * len(ADAMW_ENTRIES))()
    views = []
    for i, (n, off, has_g) in enumerate(ADAMW_ENTRIES):
        v = state(pool, n, f"{name}/{i}", off)
        table[i].p, table[i].m, table[i].v = v["p"].data_ptr(), v["m"].data_ptr(), v["v"].data_ptr()
        table[i].g = v["g"].data_ptr() if has_g else None
        table[i].n, table[i].lr, table[i].weight_decay = n, 1e-3 * (1 + i), 0.01 * i
        views.append(v)
    bmap, nb = plan(lib, [n for n, _, _ in ADAMW_ENTRIES])
    return pool, table, views, bmap, nb


def table_cases(pkg, out):
    L = pkg.lib
    lib = L.load()
    from test_kernel_edges_aux_gpu import ADAMW_ENTRIES
    clip = torch.tensor([3.3, 0.37], device=DEV)

    for max_norm in MAX_NORMS:
        for entry, scale in (("plain", None), ("scaled1", 1.0), ("scaled0.5", 0.5)):
            pool, table, _, bmap, nb = mixed_table(L, lib, "table/grad_norm")
            part, res = pool.take(nb), pool.take(2)
            if scale is None:
                L.call("sgl_op_grad_norm", DEV, upload(table).data_ptr(), bmap.data_ptr(), nb, max_norm, part.data_ptr(),
                       res.data_ptr())
            else:
                L.call("sgl_op_grad_norm_scaled", DEV, upload(table).data_ptr(), bmap.data_ptr(), nb, max_norm, scale,
                       part.data_ptr(), res.data_ptr())
            out[f"table/grad_norm/{entry}/max_norm{max_norm:g}"] = sha(pool.buf)

    pool, table, _, bmap, nb = mixed_table(L, lib, "table/ema")
    L.call("sgl_op_ema", DEV, upload(table).data_ptr(), bmap.data_ptr(), nb, 0.999)
    out["table/ema/decay0.999"] = sha(pool.buf)

    for step in (1, 1000):
        for cname, nc in (("noclip", None), ("clip0.37", clip)):
            pool, table, _, bmap, nb = mixed_table(L, lib, f"table/adamw/{step}")
            L.call("sgl_op_adamw", DEV, upload(table).data_ptr(), bmap.data_ptr(), nb, B1, B2, EPS, step, L.ptr(nc))
            out[f"table/adamw/step{step}/{cname}"] = sha(pool.buf)

            # dst_f32: aligned (entries 0, 1, 5), 4 bytes off (3), one element (4); EMA: aligned (0, 5), 4 bytes off (2),
            # aligned next to misaligned state (3); entry 5 (12289, all aligned) takes the full-chunk path with both
            pool, table, _, bmap, nb = mixed_table(L, lib, f"table/adamw_ex/{step}")
            aux = (L.SglAdamwAux * len(ADAMW_ENTRIES))()
            for i, (n, _, _) in enumerate(ADAMW_ENTRIES):
                aux[i].group = i % 2
                if i in (0, 1, 3, 4, 5):
                    aux[i].dst_f32 = pool.take(n, off=4 if i == 3 else 0).data_ptr()
                if i in (0, 2, 3, 5):
                    aux[i].ema = pool.take(n, off=4 if i == 2 else 0, init=floats((n,), f"table/ema0/{i}") - 0.5).data_ptr()
            aux[8].group = -1                                                   # the table entry's own lr / weight_decay
            hyper = (C.c_float * 4)(2e-3, 0.01, 5e-4, 0.0)
            L.call("sgl_op_adamw_ex", DEV, upload(table).data_ptr(), upload(aux).data_ptr(), bmap.data_ptr(), nb, B1, B2,
                   EPS, step, L.ptr(nc), hyper, 2, 0.9)
            out[f"table/adamw_ex/step{step}/{cname}"] = sha(pool.buf)


def tiled_cases(pkg, out):
    L = pkg.lib
    lib = L.load()
    n_all = sum(r * c for r, c, _, _ in TILED_MATS)
    for dt in (BF16, F16, F32):
        for both in (True, False):
            for ema in (True, False):
                for step in (1, 1000):
                    name = f"tiled/{DT_NAME[dt]}/{'both' if both else 'dst_only'}/{'ema' if ema else 'noema'}/step{step}"
                    st, shadows = Pool(n_all * 4 * 5 + 16384), Pool(n_all * 4 * 3 + 65536)
                    table = (L.SglAdamwTensor * len(TILED_MATS))()
                    aux = (L.SglAdamwAux * len(TILED_MATS))()
                    numel = []
                    for i, (rows, cols, row0, off) in enumerate(TILED_MATS):
                        v = state(st, rows * cols, f"tiled/{i}", off)
                        table[i].p, table[i].g, table[i].m, table[i].v = (v[k].data_ptr() for k in "pgmv")
                        table[i].n, table[i].lr, table[i].weight_decay = rows * cols, 1e-3 * (1 + i), 0.01 * i
                        a = aux[i]
                        a.rows, a.cols, a.row0, a.dtype, a.group = rows, cols, row0, dt, -1
                        a.ld, a.ld_t = rup(cols, 8) + 8, (rup(rows - row0, 8) + 8) if both else 0
                        a.dst = shadows.take((rows - row0) * a.ld, TDT[dt]).data_ptr()
                        if both:
                            a.dst_t = shadows.take(cols * a.ld_t, TDT[dt]).data_ptr()
                        if ema:
                            a.ema = st.take(rows * cols, init=floats((rows * cols,), f"tiled/ema0/{i}") - 0.5).data_ptr()
                        numel.append(((rows + 63) // 64) * ((cols + 63) // 64) * 4096)
                    bmap, nb = plan(lib, numel)
                    L.call("sgl_op_adamw_ex", DEV, upload(table).data_ptr(), upload(aux).data_ptr(), bmap.data_ptr(), nb, B1,
                           B2, EPS, step, None, None, 0, 0.9)
                    out[name + "/state"] = sha(st.buf)                  # parameters, both moments, EMA
                    out[name + "/shadows"] = sha(shadows.buf)           # both copies, padding and gaps included


def recast(model, x):
    """The model's arena after a re-cast of every unit over 0x5A bytes."""
    with torch.no_grad():
        model(pixel_values=x)                                   # allocates the arena on the first call
        model._shadows.arena.fill_(0x5A)
        model._shadows.invalidate()
        model(pixel_values=x)
    return model._shadows.arena


def model_cases(pkg, out):
    for cfg_name in MODEL_CONFIGS:
        cfg = pkg.get_config(cfg_name)
        x = (floats((2, 3, cfg.image_size, cfg.image_size), f"model/{cfg_name}/x") - 0.5).to(DEV)

        def make(mode):
            m = pkg.SiglipVisionModelHIP(cfg, compute_dtype=mode).to(DEV)
            with torch.no_grad():
                for n, p in m.named_parameters():
                    p.copy_((floats(tuple(p.shape), f"model/{cfg_name}/{n}") - 0.5) * 0.1)
            return m

        out[f"model/{cfg_name}/mxfp8/recast_arena"] = sha(recast(make("mxfp8"), x))
        for mode in TRAIN_MODES:
            model, twin = make(mode), make(mode)
            recast(model, x)
            opt = pkg.FusedAdamW(model.parameters(), lr=1e-3, weight_decay=0.01, max_grad_norm=1.0)
            opt.attach_encoder(model)
            opt.attach_ema(pkg.ExponentialMovingAverage(model, decay=0.9))
            for step in (1, 2):
                for n, p in model.named_parameters():
                    p.grad = ((floats(tuple(p.shape), f"model/{cfg_name}/{n}/g{step}") - 0.5) * 0.01).to(DEV)
                serial = model._shadows.serial
                opt.step()
                assert model._shadows.serial == serial + 1, "the step's shadows were not adopted"
                name = f"model/{cfg_name}/{mode}/step{step}"
                out[name + "/optimizer_arena"] = sha(model._shadows.arena)
                twin.load_state_dict(model.state_dict())
                out[name + "/recast_arena"] = sha(recast(twin, x))


def kernel_cases(pkg, out):
    import test_kernel_edges_internal_gpu as ti
    L = pkg.lib

    # ---- sgl_op_cast_job: every one-matrix variant over CAST_R x CAST_C in one pool per (variant, dtype), then the tables
    for dt in (BF16, F16, F32):
        tdt = TDT[dt]

        def mat(pool, R, C_, lds, Rp, Cp, ldd, ldt, off, want_dst, want_t, name):
            src = pool.take(R * lds, off=4 if off else 0, init=(floats((R, lds), name) - 0.5) * 6)
            return L.SglCastMat(src.data_ptr(), pool.take(Rp * ldd, tdt).data_ptr() if want_dst else None,
                                pool.take(Cp * ldt, tdt).data_ptr() if want_t else None, R, C_, lds, Rp, Cp, ldd, ldt)

        for variant, (off, lds, Rp, Cp, ldd, ldt, want_dst, want_t) in ti.CAST_JOB_VARIANTS.items():
            pool = Pool(24 << 20)
            for R in ti.CAST_R:
                for C_ in ti.CAST_C:
                    rp, cp = Rp(R), Cp(C_)
                    m = mat(pool, R, C_, lds(C_), rp, cp, ldd(cp), ldt(rp), off, want_dst, want_t,
                            f"cast_job/{variant}/{R}x{C_}")
                    L.call("sgl_op_cast_job", DEV, (L.SglCastMat * 1)(m), 1, None, 0, dt)
            out[f"cast_job/{variant}/{DT_NAME[dt]}"] = sha(pool.buf[:rup(pool.at, 256)])
        pool = Pool(8 << 20)
        mats = [mat(pool, R, C_, C_ + i, Rp, Cp, Cp + 8 * (i % 2), Rp + 8 * (i % 3), i % 2, True, i != 2,
                    f"cast_job/six/{i}")
                for i, (R, C_, Rp, Cp) in enumerate([(5, 7, 16, 8), (65, 33, 80, 40), (100, 70, 112, 72), (144, 538, 144, 544),
                                                     (538, 1, 544, 8), (64, 64, 64, 64)])]
        vecs = [L.SglCastVec(pool.take(max(n, 1), init=floats((max(n, 1),), f"cast_job/vec/{n}")).data_ptr(),
                             pool.take(np_).data_ptr(), n, np_) for n, np_ in ((1, 8), (144, 256), (538, 640), (257, 300))]
        L.call("sgl_op_cast_job", DEV, (L.SglCastMat * 6)(*mats), 6, (L.SglCastVec * 4)(*vecs), 4, dt)
        out[f"cast_job/six_matrices_four_vectors/{DT_NAME[dt]}"] = sha(pool.buf[:rup(pool.at, 256)])
        pool = Pool(2 << 20)
        m = mat(pool, 538, 144, 144, 640, 144, 144, 640, 0, True, True, "cast_job/hostile_fc1")
        v = L.SglCastVec(pool.take(538, init=floats((538,), "cast_job/hostile_fc1_b")).data_ptr(), pool.take(640).data_ptr(),
                         538, 640)
        L.call("sgl_op_cast_job", DEV, (L.SglCastMat * 1)(m), 1, (L.SglCastVec * 1)(v), 1, dt)
        out[f"cast_job/hostile_fc1_538_rows/{DT_NAME[dt]}"] = sha(pool.buf[:rup(pool.at, 256)])

    # ---- sgl_op_split3: values over 33 binades; whole and partial 8-chunks; the grid-stride loop's second trip
    def split_source(pool, R, C_, ld, off, name):
        i = torch.arange(R * ld, dtype=torch.int64)
        x = (floats((R * ld,), name) - 0.5) * torch.exp2(((i % 33) - 16).float())
        return pool.take(R * ld, off=4 if off else 0, init=x)

    for stacked in (0, 1):
        for b_side in (0, 1):
            pool = Pool(1 << 20)
            for C_ in (8, 9, 15, 144):
                for kind in ("aligned_ld_mod4_0", "src_4_bytes_off", "ld_mod4_1"):
                    R, Cs = 5, rup(C_, 8)
                    ld = rup(C_, 4) + (1 if kind == "ld_mod4_1" else 4)
                    src = split_source(pool, R, C_, ld, kind == "src_4_bytes_off", f"split3/{C_}/{kind}")
                    dst = pool.take(3 * R * Cs, torch.bfloat16)
                    L.call("sgl_op_split3", DEV, src.data_ptr(), R, C_, ld, dst.data_ptr(), Cs, b_side, stacked)
            out[f"split3/{'stack' if stacked else 'rows'}/{'b' if b_side else 'a'}_side"] = sha(pool.buf[:rup(pool.at, 256)])
    R, C_ = 4100, 4096
    assert R * (C_ // 8) > 8192 * 256
    pool = Pool(R * C_ * 4 + 4096)
    src = split_source(pool, R, C_, C_, False, "split3/grid_stride")
    for stacked, b_side in ((0, 1), (1, 0)):
        dst = Pool(3 * R * C_ * 2 + 4096)
        L.call("sgl_op_split3", DEV, src.data_ptr(), R, C_, C_, dst.take(3 * R * C_, torch.bfloat16).data_ptr(), C_, b_side,
               stacked)
        out[f"split3/grid_stride/{'stack' if stacked else 'rows'}"] = sha(dst.buf)


def digests(pkg) -> dict:
    """case name -> SHA-256, for every case of the file's docstring."""
    out = {}
    for family in (table_cases, tiled_cases, model_cases, kernel_cases):
        family(pkg, out)
        torch.cuda.synchronize()
        _KEEP.clear()
    return out


def twins(d):
    """Pairs of case names that must carry the same digest WITHIN one tree: sgl_op_grad_norm and sgl_op_grad_norm_scaled at
    scale 1; the arena the optimizer wrote and the arena a fresh re-cast of the same parameters writes."""
    pairs = [(n, n.replace("/plain/", "/scaled1/")) for n in d if n.startswith("table/grad_norm/plain/")]
    pairs += [(n, n.replace("/optimizer_arena", "/recast_arena")) for n in d if n.endswith("/optimizer_arena")]
    return pairs


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
    for a, b in twins(d):
        print(f"[twin] {'same' if d[a] == d[b] else 'DIFFERENT'}: {a} | {b}")


if __name__ == "__main__":
    main()
