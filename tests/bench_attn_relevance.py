"""What gradient-weighted attention relevance costs (so400m-patch14-384, bf16, B = 1 and B = 42, the app's view batch).
One process, event-timed, warmed up, medians of --steps runs.  Not collected by pytest; bench.py is the flagship benchmark
and does not know about this.

Routes  a  the attack step alone: saving forward + backward to the pixels of a frozen encoder (score = pooler_output[:, 1])
        r  model.attention_relevance of the same score: the same forward + backward with one sgl_op_attn_grad_probs launch
           (RELEVANCE, HEAD_MEAN) inside each of the 27 blocks' backward steps, the pooling head's map, and 27 row-vector
           bmm (B,1,729) x (B,729,729)
        k  the 27 kernel calls alone on operands of the model's shapes (q, k, v (B,16,729,80) bf16, dO (B*729,1152) bf16,
           lse (B,16,729)): per image and layer 2 * 2 * H * N^2 * DP = 2.7 GFLOP, N^2 * 4 = 2.1 MB written
        t  the same 27 maps by torch on the GPU from the same operands:
           relu(softmax(q k^T * scale, -1) * (dO v^T)).mean(1)
Peak memory (torch.cuda.max_memory_allocated over the timed runs, less what was allocated before them) of every route.

No time is fixed in advance and no ratio is asserted.  Prints ONE JSON line; --out writes it.  --headline A B embeds two
files holding bench.py's JSON line (the parent commit's and this tree's, measured in the same session).

    python tests/bench_attn_relevance.py [--steps 10] [--warmup 2] [--out profiles/attn_relevance_bench.json]
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


def last_json_line(path):
    with open(path) as f:
        lines = [l for l in f.read().splitlines() if l.startswith("{")]
    return json.loads(lines[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 42])
    ap.add_argument("--headline", nargs=2, default=None, metavar=("PARENT", "THIS"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    pkg = entry.load_package()
    pkg.lib.load()
    cfg = pkg.get_config("so400m-patch14-384")
    model = pkg.SiglipVisionModelHIP(cfg, compute_dtype="bf16").to("cuda")
    model.load_state_dict(pkg.weights.seeded_state_dict(cfg, seed=0))
    model.requires_grad_(False)
    L, H, D, S = cfg.num_hidden_layers, cfg.num_attention_heads, cfg.hidden_size, cfg.image_size
    dh = D // H
    DP = (dh + 15) // 16 * 16
    N = (S // cfg.patch_size) ** 2
    st = torch.cuda.current_stream()
    score = lambda o: o.pooler_output[:, 1]
    res = {"config": "so400m-patch14-384", "compute_dtype": "bf16", "layers": L, "heads": H, "tokens": N, "head_dim": dh,
           "device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup, "batches": {}}
    for B in args.batches:
        x = pkg.weights.seeded_pixels(B, S, S, seed=3).cuda()
        g = torch.Generator(device="cuda").manual_seed(B)
        q, k, v = (torch.zeros(B, H, N, DP, dtype=torch.bfloat16, device="cuda") for _ in range(3))
        for t in (q, k, v):
            t[..., :dh] = torch.randn(B, H, N, dh, generator=g, device="cuda").to(torch.bfloat16)
        dout = torch.randn(B * N, H * dh, generator=g, device="cuda").to(torch.bfloat16)
        scale = dh ** -0.5
        lse = torch.logsumexp((q.float() @ k.float().transpose(-1, -2)) * scale, -1).contiguous()
        out = torch.empty(B, N, N, dtype=torch.float32, device="cuda")
        dout_h = dout.view(B, N, H, dh).permute(0, 2, 1, 3)

        def route_a():
            xg = x.detach().clone().requires_grad_(True)
            torch.autograd.grad(score(model(pixel_values=xg)).sum(), xg)

        def route_r():
            model.attention_relevance(x, score, interpolate_pos_encoding=False)

        def route_k():
            for _ in range(L):
                pkg.lib.call("sgl_op_attn_grad_probs", q.device, pkg.lib.SGL_DTYPE_BF16, q.data_ptr(), k.data_ptr(),
                             v.data_ptr(), dout.data_ptr(), lse.data_ptr(), out.data_ptr(), B, H, N, dh, DP,
                             pkg.lib.ATTN_GRAD_RELEVANCE, pkg.lib.ATTN_PROBS_HEAD_MEAN)

        def route_t():
            for _ in range(L):
                p = torch.softmax((q @ k.transpose(-1, -2)).float() * scale, -1)
                torch.relu(p * (dout_h @ v[..., :dh].transpose(-1, -2)).float()).mean(1)

        r = {}
        for name, fn in (("a_attack_step", route_a), ("r_attention_relevance", route_r), ("k_27_maps_hip", route_k),
                         ("t_27_maps_torch", route_t)):
            timed(fn, args.warmup, st)
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            r[name] = stats(timed(fn, args.steps, st))
            r[name]["peak_extra_MB"] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
        per_map_s = r["k_27_maps_hip"]["ms_median"] * 1e-3 / (L * B)
        r["k_per_image_layer"] = {"us": round(per_map_s * 1e6, 2),
                                  "write_GBps": round(N * N * 4 / per_map_s * 1e-9, 1),
                                  "TFLOPs": round(4 * H * N * N * DP / per_map_s * 1e-12, 2)}
        r["r_over_a"] = round(r["r_attention_relevance"]["ms_median"] / r["a_attack_step"]["ms_median"], 3)
        r["t_over_k"] = round(r["t_27_maps_torch"]["ms_median"] / r["k_27_maps_hip"]["ms_median"], 3)
        res["batches"][str(B)] = r
        del q, k, v, dout, dout_h, lse, out, x
        torch.cuda.empty_cache()
    if args.headline:
        res["headline_bench_py"] = {"parent_commit": last_json_line(args.headline[0]),
                                    "this_tree_no_capture": last_json_line(args.headline[1])}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
