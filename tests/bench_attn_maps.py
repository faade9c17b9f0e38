"""What attention maps cost (so400m-patch14-384, bf16, B = 1 and B = 42, the app's view batch).  One process, event-timed,
warmed up, medians.  Not collected by pytest; bench.py is the flagship benchmark and does not know about this.

Routes  a  the inference forward (no maps), under no_grad
        b  model.attention_rollout: the saving forward + 27 head-mean maps (sgl_attention_probs, HEAD_MEAN) + the probe map
           + heads.attention_rollout (27 bmm of (B,729,729))
        m  the 27 head-mean maps alone, one sgl_op_attn_probs launch per layer on operands of the model's shapes
           (q, k (B,16,729,80) bf16, lse (B,16,729)): per image and layer it writes N^2 * 4 = 2.1 MB, reads
           2 * H * N * DP * 2 = 3.7 MB and does 2 * H * N^2 * DP = 1.4 GFLOP (figures to compare against, not targets)
        c  the same 27 maps by torch on the GPU from the same operands: softmax(q k^T * scale, -1).mean(1)

No time is fixed in advance and no ratio is asserted.  Prints ONE JSON line; --out writes it.

    python tests/bench_attn_maps.py [--steps 5] [--warmup 2] [--out profiles/attn_maps_bench.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402
from bench_input_grad import median, timed  # noqa: E402


def stats(t, nd=3):
    return {"ms_median": round(median(t), nd), "ms_min": round(min(t), nd), "ms_max": round(max(t), nd), "n": len(t)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 42])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    pkg = entry.load_package()
    lib = pkg.lib.load()
    cfg = pkg.get_config("so400m-patch14-384")
    model = pkg.SiglipVisionModelHIP(cfg, compute_dtype="bf16").to("cuda")
    model.load_state_dict(pkg.weights.seeded_state_dict(cfg, seed=0))
    model.requires_grad_(False)
    L, H, D, S = cfg.num_hidden_layers, cfg.num_attention_heads, cfg.hidden_size, cfg.image_size
    dh = D // H
    DP = (dh + 15) // 16 * 16
    N = (S // cfg.patch_size) ** 2
    st = torch.cuda.current_stream()
    res = {"config": "so400m-patch14-384", "compute_dtype": "bf16", "layers": L, "heads": H, "tokens": N, "head_dim": dh,
           "device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup, "batches": {}}
    for B in args.batches:
        x = pkg.weights.seeded_pixels(B, S, S, seed=3).cuda()
        g = torch.Generator(device="cuda").manual_seed(B)
        q = torch.zeros(B, H, N, DP, dtype=torch.bfloat16, device="cuda")
        k = torch.zeros_like(q)
        q[..., :dh] = torch.randn(B, H, N, dh, generator=g, device="cuda").to(torch.bfloat16)
        k[..., :dh] = torch.randn(B, H, N, dh, generator=g, device="cuda").to(torch.bfloat16)
        scale = dh ** -0.5
        lse = torch.logsumexp((q.float() @ k.float().transpose(-1, -2)) * scale, -1).contiguous()
        out = torch.empty(B, N, N, dtype=torch.float32, device="cuda")

        def route_a():
            with torch.no_grad():
                model(pixel_values=x)

        def route_b():
            model.attention_rollout(x)

        def route_m():
            for _ in range(L):
                pkg.lib.call("sgl_op_attn_probs", q.device, pkg.lib.SGL_DTYPE_BF16, q.data_ptr(), k.data_ptr(),
                             lse.data_ptr(), out.data_ptr(), B, H, N, dh, DP, pkg.lib.ATTN_PROBS_HEAD_MEAN)

        def route_c():
            for _ in range(L):
                torch.softmax((q @ k.transpose(-1, -2)).float() * scale, -1).mean(1)

        r = {}
        for name, fn in (("a_inference_forward", route_a), ("b_rollout", route_b), ("m_head_mean_maps_hip", route_m),
                         ("c_head_mean_maps_torch", route_c)):
            timed(fn, args.warmup, st)
            r[name] = stats(timed(fn, args.steps, st))
        per_map_s = r["m_head_mean_maps_hip"]["ms_median"] * 1e-3 / (L * B)
        r["m_per_image_layer"] = {"us": round(per_map_s * 1e6, 2),
                                  "write_GBps": round(N * N * 4 / per_map_s * 1e-9, 1),
                                  "read_GBps": round(2 * H * N * DP * 2 / per_map_s * 1e-9, 1),
                                  "TFLOPs": round(2 * H * N * N * DP / per_map_s * 1e-12, 2)}
        r["b_over_a"] = round(r["b_rollout"]["ms_median"] / r["a_inference_forward"]["ms_median"], 3)
        r["c_over_m"] = round(r["c_head_mean_maps_torch"]["ms_median"] / r["m_head_mean_maps_hip"]["ms_median"], 3)
        res["batches"][str(B)] = r
        del q, k, lse, out, x
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
