"""What one validation batch of the mask localisation metrics costs (SID configuration: so400m@384, g = 27, S = 384, B = 64;
also base@224, g = 14, S = 224, B = 256; every image masked).  One process, event-timed, warmed up, medians; the two GPU
routes alternate in blocks.

Routes  a  the best route WITHOUT sgl_op_seg_eval, kept entirely on the GPU (generous to it: the reference copies to the
           host): F.interpolate to (B,1,S,S), then per cut `z > cut`, per-image sums, Dice / IoU / TP / FP / FN accumulated
           into device tensors, for the 17 cuts of the default sweep (mask_thr 0.5 is one of them); no host copy, and NO
           pixel AUC (so it does less than b)
        b  heads.MaskMetrics.update on the low-res logits: one sgl_op_seg_eval launch (uint8 or fp32 masks) plus the ops
           on (B, K+1) integers, INCLUDING the 4096-bin AUC histogram
        k  the sgl_op_seg_eval launch alone, for the achieved bytes/s (memory bandwidth is the bound: the mask is the only
           traffic that scales)
        h  for orientation only, ON THE CPU at B = 1, S = 384: the reference's host route written out literally (`.cpu()`
           copies, 17 passes + 17 sklearn f1_score calls, the per-pixel reservoir loop, timed over its first
           `--reservoir-iters` iterations and scaled to the 147 456 of one image); skipped where sklearn is missing

No time is fixed in advance; what must hold is b <= a at both shapes in the same run, recorded as `b_le_a`.  Prints ONE JSON
line; --out writes it.

    python tests/bench_seg_eval.py [--blocks 5] [--steps 5] [--warmup 3] [--out profiles/seg_eval_bench.json]
"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402
from bench_input_grad import median, timed  # noqa: E402

SHAPES = [(64, 27, 384), (256, 14, 224)]       # (B, g, S)


def stats(t, nd=4):
    return {"ms_median": round(median(t), nd), "ms_min": round(min(t), nd), "ms_max": round(max(t), nd), "n": len(t)}


def make_batch(B, g, S, seed):
    gen = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(S), torch.arange(S), indexing="ij")
    c = torch.rand(B, 2, generator=gen) * 0.6 + 0.2
    r = torch.rand(B, 2, generator=gen) * 0.2 + 0.1
    masks = ((((yy[None] - c[:, 0, None, None] * S) / (r[:, 0, None, None] * S)) ** 2
              + ((xx[None] - c[:, 1, None, None] * S) / (r[:, 1, None, None] * S)) ** 2) <= 1.0).float()[:, None]
    lr = F.adaptive_avg_pool2d(masks, (g, g)) * 4.0 - 1.4 + torch.randn(B, 1, g, g, generator=gen)
    return lr.cuda(), masks.cuda()


class TorchRoute:
    """Route a: full-resolution logits and elementwise passes per cut, state on the device."""

    def __init__(self, cuts, eps=1e-6):
        self.cuts, self.eps = [float(c) for c in cuts], eps
        K = len(self.cuts)
        self.cnt = torch.zeros(3, K, dtype=torch.int64, device="cuda")
        self.sums = torch.zeros(2, K, dtype=torch.float64, device="cuda")

    def update(self, lr, masks):
        z = F.interpolate(lr, size=masks.shape[-2:], mode="bilinear", align_corners=False)
        tsum = masks.sum(dim=(1, 2, 3))
        for j, cut in enumerate(self.cuts):
            p = (z > cut).float()
            inter = (p * masks).sum(dim=(1, 2, 3))
            psum = p.sum(dim=(1, 2, 3))
            self.sums[0, j] += (2 * inter / (psum + tsum + self.eps)).sum()
            self.sums[1, j] += (inter / (psum + tsum - inter + self.eps)).sum()
            self.cnt[0, j] += inter.sum().long()
            self.cnt[1, j] += (psum - inter).sum().long()
            self.cnt[2, j] += (tsum - inter).sum().long()


def host_route(lr, masks, reservoir_iters):
    """Route h: what the reference's validation loop does with one image's logits, on the CPU."""
    from sklearn.metrics import f1_score
    out = {}
    t0 = time.perf_counter()
    z = F.interpolate(lr, size=masks.shape[-2:], mode="bilinear", align_corners=False)
    logits_list, masks_list = [z.detach().cpu()], [masks.detach().cpu()]
    out["copies_ms"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    all_l, all_m = torch.cat(logits_list), torch.cat(masks_list)
    for thr in np.linspace(0.1, 0.9, 17):
        p = (torch.sigmoid(all_l) > thr).float()
        inter = (p * all_m).sum(dim=(1, 2, 3))
        union = (p + all_m - p * all_m).sum(dim=(1, 2, 3)) + 1e-6
        (2 * inter / (p.sum(dim=(1, 2, 3)) + all_m.sum(dim=(1, 2, 3)) + 1e-6)).tolist()
        (inter / union).tolist()
        f1_score(all_m.flatten().numpy(), p.flatten().numpy(), zero_division=0)
    out["sweep_17_ms"] = (time.perf_counter() - t0) * 1e3
    # the per-pixel reservoir update of a full 400 000-pixel buffer
    buf_l, buf_t = torch.randn(400_000), torch.zeros(400_000)
    l, t = all_l.flatten(), all_m.flatten()
    count = 400_000
    t0 = time.perf_counter()
    for i in range(reservoir_iters):
        count += 1
        j = random.randint(0, count - 1)
        if j < 400_000:
            buf_l[j] = l[i]
            buf_t[j] = t[i]
    per_iter = (time.perf_counter() - t0) / reservoir_iters
    out["reservoir_loop_ms_scaled"] = per_iter * l.numel() * 1e3
    out["reservoir_iters_timed"] = reservoir_iters
    out["total_ms"] = out["copies_ms"] + out["sweep_17_ms"] + out["reservoir_loop_ms_scaled"]
    return {k: round(v, 3) if isinstance(v, float) else v for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reservoir-iters", type=int, default=20000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_seg_eval.py measures on the GPU only"
    pkg = entry.load_package()
    lib = pkg.lib.load()
    st = torch.cuda.current_stream()
    NB = pkg.lib.SEG_EVAL_AUC_BINS
    result = {"bench": "seg_eval", "device": torch.cuda.get_device_name(0), "bound": "memory bandwidth (the mask read)",
              "blocks": args.blocks, "steps": args.steps, "warmup": args.warmup, "shapes": []}
    for B, g, S in SHAPES:
        lr, masks = make_batch(B, g, S, seed=B + S)
        masks_u8 = masks.to(torch.uint8)
        mm = pkg.MaskMetrics()
        K = len(mm.cuts)
        cuts = mm.device_cuts("cuda:0")
        route_a = TorchRoute(mm.cuts)
        mm_u8 = pkg.MaskMetrics()
        hist = torch.empty(B, 2, K + 1, dtype=torch.int32, device="cuda")
        auc = torch.zeros(2, NB, dtype=torch.int64, device="cuda")
        lr32 = lr.reshape(B, g, g).contiguous()

        def kernel(t, code):
            s = lib.sgl_op_seg_eval(lr32.data_ptr(), t.data_ptr(), code, None, cuts.data_ptr(), K, hist.data_ptr(),
                                    auc.data_ptr(), B, g, S, st.cuda_stream)
            assert s == 0, s
        legs = {"a_torch_fullres_17cuts": lambda: route_a.update(lr, masks),
                "b_maskmetrics_update_f32mask": lambda: mm.update(lr, masks),
                "b_maskmetrics_update_u8mask": lambda: mm_u8.update(lr, masks_u8),
                "k_kernel_f32mask": lambda: kernel(masks, pkg.lib.SGL_DTYPE_F32),
                "k_kernel_u8mask": lambda: kernel(masks_u8, pkg.lib.SGL_DTYPE_U8)}
        for fn in legs.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in legs}
        for _ in range(args.blocks):                 # the routes alternate: a b b k k a b b k k ...
            for name, fn in legs.items():
                times[name] += timed(fn, args.steps, st)
        # the two routes agree on the counts they share (route a has no AUC)
        fresh, ref = pkg.MaskMetrics(), TorchRoute(mm.cuts)
        fresh.update(lr, masks)
        ref.update(lr, masks)
        s = fresh.state()
        pix = B * S * S
        mism = int((s["tp"] - ref.cnt[0]).abs().max().item())
        entry_ = {"B": B, "g": g, "S": S, "K": K, "legs": {k: stats(v) for k, v in times.items()},
                  "max_tp_count_difference_a_vs_b": mism, "pixels": pix}
        for tag, esz in (("f32mask", 4), ("u8mask", 1)):
            nbytes = pix * esz + B * g * g * 4 + B * 2 * (K + 1) * 4 + 2 * NB * 8
            ms = median(times["k_kernel_" + tag])
            entry_["kernel_" + tag] = {"algorithmic_bytes": nbytes, "achieved_GBps": round(nbytes / ms / 1e6, 1),
                                       "Gpixel_per_s": round(pix / ms / 1e6, 2)}
        a = median(times["a_torch_fullres_17cuts"])
        entry_["b_le_a"] = {k: bool(median(times[k]) <= a) for k in times if k.startswith("b_")}
        entry_["a_over_b"] = {k: round(a / median(times[k]), 2) for k in times if k.startswith("b_")}
        result["shapes"].append(entry_)
        del route_a, mm, mm_u8, fresh, ref, lr, masks, masks_u8
        torch.cuda.empty_cache()
    try:
        torch.manual_seed(0)
        lr1, m1 = make_batch(1, 27, 384, seed=1)
        result["h_reference_host_route_cpu_B1_S384_orientation_only"] = dict(
            host_route(lr1.cpu(), m1.cpu(), args.reservoir_iters), cpus=len(os.sched_getaffinity(0)),
            note="CPU, one image; reservoir loop scaled from the timed iterations; not comparable with the GPU legs")
    except ImportError as e:
        result["h_reference_host_route_cpu_B1_S384_orientation_only"] = f"not measured ({e})"
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
