"""What the app's test-time views cost: so400m-patch14-384, bf16 inference, one uint8 source image, the 42 views of
`preprocess.detect_views` (9 crops, the rotated frame, 16 grid cells each with its rotated view), for sources of
1024 x 1024 and 2048 x 1365.  One process, event-timed, warmed up, medians; the two GPU routes alternate in blocks.

Legs:  a  sgl_op_preprocess_views alone, patch-major bf16 (the encoder's operand) and NCHW fp32 (the pixel tensor)
       b  the only route without it: per window a contiguous cropped copy + one sgl_op_preprocess, 42 copies and 42
          launches into slices of one operand.  That route has NO rotated view: the 17 rotated windows are replaced by
          their unrotated crops (the same pixels read, so the same cost), and its output is not the app's
       c  the encoder forward at V = 42 from patches= (what the transform feeds)
       d  where PIL is importable, the reference's host route: crop / rotate / resize(384, BILINEAR) / to-tensor /
          normalise per window, stack, upload; a host clock round work that ends in a device synchronise, with the
          number of CPUs the process may use

No time is fixed in advance; whether (a) beats (b) is recorded as it comes out.  Prints ONE JSON line; --out writes it.

    python tests/bench_views.py [--blocks 4] [--steps 10] [--warmup 3] [--out profiles/views_bench.json]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402
from bench_input_grad import median, timed  # noqa: E402

SOURCES = [(1024, 1024), (2048, 1365)]       # (w, h)


def stats(t, nd=4):
    return {"ms_median": round(median(t), nd), "ms_min": round(min(t), nd), "ms_max": round(max(t), nd)}


def pil_route(Image, np, img_hwc, views, S, device):
    pil = Image.fromarray(img_hwc)
    rows = []
    for v in views:
        c = pil.crop(v.box)
        if v.turns:
            c = c.rotate(90 * v.turns, expand=not v.keep_canvas)
        t = torch.from_numpy(np.asarray(c.resize((S, S), Image.BILINEAR)).copy()).permute(2, 0, 1).float().div_(255.0)
        rows.append((t - 0.5) / 0.5)
    return torch.stack(rows).to(device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", default="so400m-patch14-384")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_views.py measures on the GPU only"
    pkg = entry.load_package()
    lib = pkg.lib.load()
    pp = pkg.preprocess
    cfg = pkg.get_config(args.config)
    S, P = cfg.image_size, cfg.patch_size
    Kp = (3 * P * P + 63) // 64 * 64
    g = S // P
    dev = torch.device("cuda")
    st = torch.cuda.current_stream()
    s = pkg.lib.current_stream_handle(dev)
    model = pkg.SiglipVisionModelHIP(cfg, compute_dtype="bf16")
    model.load_state_dict(pkg.weights.seeded_state_dict(cfg, seed=0))
    model = model.cuda().eval().requires_grad_(False)
    try:
        from PIL import Image
        import numpy as np
    except ImportError:
        Image = np = None

    res = {"metric": f"{args.config} bf16 inference: the app's 42 test-time views of one uint8 image, transform routes and "
                     "the encoder forward they feed; one process, event-timed medians, GPU routes alternating in blocks",
           "views": 42, "size": S, "blocks": args.blocks, "steps_per_block": args.steps, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(0),
           "parent_route_note": "leg b has no rotated view: the 17 rotated windows are replaced by their unrotated crops",
           "sources": []}
    for w, h in SOURCES:
        gen = torch.Generator().manual_seed(w + h)
        img = torch.randint(0, 256, (1, h, w, 3), generator=gen, dtype=torch.uint8)
        src = img.cuda()
        d = pp.detect_views(h, w)
        views = d.views
        V = len(views)
        assert V == 42
        tab = pp.view_table(views, 1, h, w)
        op = torch.empty(V * g * g, Kp, device=dev, dtype=torch.bfloat16)
        op_b = torch.empty_like(op)
        px = torch.empty(V, 3, S, S, device=dev, dtype=torch.float32)
        row_bytes = g * g * Kp * 2

        def views_patch():
            assert lib.sgl_op_preprocess_views(src.data_ptr(), 1, 1, h, w, tab, V, op.data_ptr(), pkg.lib.SGL_DTYPE_BF16, S,
                                               P, Kp, 1, 0.5, 0.5, None, 0, s) == 0

        def views_nchw():
            assert lib.sgl_op_preprocess_views(src.data_ptr(), 1, 1, h, w, tab, V, px.data_ptr(), pkg.lib.SGL_DTYPE_F32, S,
                                               1, 3, 0, 0.5, 0.5, None, 0, s) == 0

        def parent_route():
            for n, v in enumerate(views):
                x0, y0, x1, y1 = v.box
                cut = src[:, y0:y1, x0:x1].contiguous()
                assert lib.sgl_op_preprocess(cut.data_ptr(), 1, 1, y1 - y0, x1 - x0, op_b.data_ptr() + n * row_bytes,
                                             pkg.lib.SGL_DTYPE_BF16, S, P, Kp, 1, 0.5, 0.5, None, 1.0, s) == 0

        legs = {"a_views_patch_major_bf16": views_patch, "a_views_nchw_f32": views_nchw,
                "b_parent_42_copies_42_launches": parent_route}
        names = list(legs)
        for n in names:
            for _ in range(args.warmup):
                legs[n]()
        torch.cuda.synchronize()
        times = {n: [] for n in names}
        for blk in range(args.blocks):
            for n in (names if blk % 2 == 0 else names[::-1]):
                times[n] += timed(legs[n], args.steps, st)
        plain = [n for n, v in enumerate(views) if v.turns == 0]       # the rows both routes define: they must agree
        rows = torch.cat([torch.arange(n * g * g, (n + 1) * g * g) for n in plain]).to(dev)
        entry_ = {"source_wh": [w, h], "plain_rows_equal_bitwise": bool(torch.equal(op[rows], op_b[rows]))}
        for n in names:
            entry_[n] = stats(times[n])
        a, b = entry_["a_views_patch_major_bf16"]["ms_median"], entry_["b_parent_42_copies_42_launches"]["ms_median"]
        entry_["b_over_a"] = round(b / a, 3)
        entry_["a_faster_than_b"] = bool(a < b)
        entry_["a_patch_major_bytes_written"] = op.numel() * 2
        entry_["a_patch_major_write_GB_per_s"] = round(op.numel() * 2 / (a * 1e-3) / 1e9, 1)

        operand = pp.PatchOperand(op, V, S, S)

        def encoder():
            with torch.no_grad():
                model(patches=operand)
        for _ in range(args.warmup):
            encoder()
        entry_["c_encoder_forward_V42_from_patches"] = stats(timed(encoder, args.steps, st), 3)

        if Image is not None:
            hwc = img[0].numpy()
            host = []
            for i in range(2 + 5):
                t0 = time.perf_counter()
                pil_route(Image, np, hwc, views, S, dev)
                torch.cuda.synchronize()
                if i >= 2:
                    host.append((time.perf_counter() - t0) * 1e3)
            entry_["d_pil_host_route"] = dict(stats(host, 2), cpus_in_affinity_mask=len(os.sched_getaffinity(0)),
                                              torch_threads=torch.get_num_threads(), runs=len(host),
                                              note="the per-window loop is the app's: one Python thread, PIL releases no work "
                                                   "to the other cores")
        else:
            entry_["d_pil_host_route"] = "not measured: PIL is not importable"
        res["sources"].append(entry_)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
