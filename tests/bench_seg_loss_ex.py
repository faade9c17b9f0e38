"""What forward + backward of the SID enhanced segmentation loss costs (so400m@384: B = 64, g = 27, S = 384; base@224:
B = 256, g = 14, S = 224; every image masked).  One process, event-timed, warmed up, medians; the routes alternate in blocks.

Routes  a  heads.combined_loss_from_lowres with all six weights non-zero (sgl_op_seg_loss_ex_fwd / _bwd, terms = 7)
        b  the same with the reference's IoU-focused weights (focal / boundary / morph 0: terms = 0)
        c  the route without the kernels: F.interpolate to (B,1,S,S) + heads.combined_segmentation_loss under autograd, fp32
        d  heads.bce_dice_loss_from_lowres, the floor (two of the six terms)
        k  the forward + backward launches alone for a, b and d (no fold, no composition, no autograd bookkeeping): at these
           sizes a, b and d are a few dozen small launches each, so their times are mostly launch overhead

Each leg is loss + backward to the (B,1,g,g) logits.  No speed-up is fixed in advance; the ratios a/c, b/c and a/d and the
peak-memory deltas (torch.cuda.max_memory_allocated over one forward + backward, above what is allocated before it) of a
and c are what is reported.  Prints ONE JSON line; --out writes it.

    python tests/bench_seg_loss_ex.py [--blocks 5] [--steps 20] [--warmup 3] [--out profiles/seg_loss_ex_bench.json]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402
from bench_input_grad import median, timed  # noqa: E402
from bench_seg_eval import make_batch, stats  # noqa: E402

SHAPES = [(64, 27, 384), (256, 14, 224)]       # (B, g, S)
ALL_SIX = dict(bce_w=0.4, focal_w=0.3, dice_w=0.5, boundary_w=0.4, iou_w=0.4, morph_w=0.2)
IOU_FOCUSED = dict(bce_w=0.14, focal_w=0.0, dice_w=0.24, boundary_w=0.0, iou_w=1.5, morph_w=0.0)


def peak_delta(fn, lr):
    lr.grad = None
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_seg_loss_ex.py measures on the GPU only"
    pkg = entry.load_package()
    lib = pkg.lib.load()
    H = pkg.heads
    st = torch.cuda.current_stream()
    result = {"bench": "seg_loss_ex", "device": torch.cuda.get_device_name(0), "blocks": args.blocks, "steps": args.steps,
              "warmup": args.warmup, "what": "loss + backward to the (B,1,g,g) logits, ms", "shapes": []}
    for B, g, S in SHAPES:
        lr0, masks = make_batch(B, g, S, seed=B + S)
        lr = lr0.clone().requires_grad_(True)

        def leg(loss_fn):
            def run():
                lr.grad = None
                loss_fn().backward()
            return run

        def torch_route():
            up = F.interpolate(lr, size=(S, S), mode="bilinear", align_corners=False)
            return H.combined_segmentation_loss(up, masks, **ALL_SIX)

        # the two launches alone (no fold, no composition of the sums, no autograd bookkeeping)
        lr32, t32 = lr0.reshape(B, g, g).contiguous(), masks.reshape(B, S, S).contiguous()
        chunks = lib.sgl_op_seg_loss_chunks(S)
        partial = torch.empty(B, chunks, 8, device="cuda")
        lib.sgl_op_seg_loss_ex_fwd(lr32.data_ptr(), t32.data_ptr(), partial.data_ptr(), B, g, S, 7, 0.25, st.cuda_stream)
        sums = partial.sum(1).contiguous()
        coef = torch.full((B, 6), 1e-6, device="cuda")
        dlr = torch.empty_like(lr32)

        def kernels(terms):
            def run():
                s1 = lib.sgl_op_seg_loss_ex_fwd(lr32.data_ptr(), t32.data_ptr(), partial.data_ptr(), B, g, S, terms, 0.25,
                                                st.cuda_stream)
                s2 = lib.sgl_op_seg_loss_ex_bwd(lr32.data_ptr(), t32.data_ptr(), sums.data_ptr(), coef.data_ptr(),
                                                dlr.data_ptr(), B, g, S, terms, 0.25, 1e-6, 1e-6, st.cuda_stream)
                assert s1 == 0 and s2 == 0, (s1, s2)
            return run

        def kernels_bce_dice():
            s1 = lib.sgl_op_seg_loss_fwd(lr32.data_ptr(), t32.data_ptr(), partial.data_ptr(), B, g, S, st.cuda_stream)
            s2 = lib.sgl_op_seg_loss_bwd(lr32.data_ptr(), t32.data_ptr(), sums.data_ptr(), coef.data_ptr(), dlr.data_ptr(),
                                         B, g, S, 1e-6, st.cuda_stream)
            assert s1 == 0 and s2 == 0, (s1, s2)

        legs = {"a_fused_all_six": leg(lambda: H.combined_loss_from_lowres(lr, masks, **ALL_SIX)),
                "b_fused_iou_focused": leg(lambda: H.combined_loss_from_lowres(lr, masks, **IOU_FOCUSED)),
                "c_torch_upsample_combined": leg(torch_route),
                "d_fused_bce_dice": leg(lambda: H.bce_dice_loss_from_lowres(lr, masks)),
                "k_kernels_all_six": kernels(7), "k_kernels_iou_focused": kernels(0), "k_kernels_bce_dice": kernels_bce_dice}
        for fn in legs.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in legs}
        for _ in range(args.blocks):                 # the routes alternate: a b c d k k k a b ...
            for name, fn in legs.items():
                times[name] += timed(fn, args.steps, st)
        # the two routes compute the same loss and gradient
        legs["a_fused_all_six"]()
        ga, la = lr.grad.clone(), H.combined_loss_from_lowres(lr, masks, **ALL_SIX).item()
        legs["c_torch_upsample_combined"]()
        gc, lc = lr.grad.clone(), torch_route().item()
        med = {k: median(v) for k, v in times.items()}
        entry_ = {"B": B, "g": g, "S": S, "legs": {k: stats(v) for k, v in times.items()},
                  "a_over_c": round(med["a_fused_all_six"] / med["c_torch_upsample_combined"], 4),
                  "b_over_c": round(med["b_fused_iou_focused"] / med["c_torch_upsample_combined"], 4),
                  "a_over_d": round(med["a_fused_all_six"] / med["d_fused_bce_dice"], 3),
                  "kernels_all_six_over_kernels_bce_dice": round(med["k_kernels_all_six"] / med["k_kernels_bce_dice"], 3),
                  "a_faster_than_c": bool(med["a_fused_all_six"] < med["c_torch_upsample_combined"]),
                  "peak_memory_delta_bytes": {"a_fused_all_six": peak_delta(legs["a_fused_all_six"], lr),
                                              "c_torch_upsample_combined": peak_delta(legs["c_torch_upsample_combined"], lr)},
                  "fullres_logits_bytes": B * S * S * 4,
                  "loss_a": la, "loss_c": lc,
                  "max_grad_difference_a_vs_c_over_max_grad": (ga - gc).abs().max().item() / gc.abs().max().item()}
        result["shapes"].append(entry_)
        del lr, lr0, masks, ga, gc
        torch.cuda.empty_cache()
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
