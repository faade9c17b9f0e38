"""bf16 vs fp16 compute mode, same process: so400m-patch14-384 training forward + backward at B = 128.

Both encoders live in one process and are timed in alternating blocks of event-timed steps after a warm-up, so that
clock drift (DVFS) and allocator state hit both modes alike.  The step is the one bench.py times (forward, mean-square
pooled loss, backward, every trainable shadow re-cast).  Prints ONE JSON line: img/s per mode (median of the per-step
times, with the min-max spread), fp16/bf16 ratio, and each mode's pooled-output error against the fp32 CPU oracle at B=2.

    python tests/bench_fp16.py [--batch 128] [--blocks 4] [--steps 5] [--warmup 3]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402


def median(v):
    v = sorted(v)
    n = len(v)
    return v[n // 2] if n % 2 else 0.5 * (v[n // 2 - 1] + v[n // 2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    pkg, oracle = entry.load_package(), entry.load_oracle()
    pkg.lib.load()
    cfg = pkg.get_config("so400m-patch14-384")
    sd = pkg.weights.seeded_state_dict(cfg, seed=0)
    modes = ("bf16", "fp16")
    models = {}
    for m in modes:
        model = pkg.SiglipVisionModelHIP(cfg, compute_dtype=m)
        model.load_state_dict(sd)
        models[m] = model.cuda()
    x = pkg.weights.seeded_pixels(args.batch, 384, 384, seed=1).cuda()
    st = torch.cuda.current_stream()

    def step(model):
        params = list(model.parameters())
        torch.autograd.graph.increment_version(params)   # as bench.py: every shadow is re-cast each step
        out = model(pixel_values=x, interpolate_pos_encoding=True)
        out.pooler_output.square().mean().backward()
        for p in params:
            p.grad = None

    for m in modes:
        for _ in range(args.warmup):
            step(models[m])
    torch.cuda.synchronize()
    times = {m: [] for m in modes}
    for blk in range(args.blocks):
        order = modes if blk % 2 == 0 else modes[::-1]
        for m in order:
            evs = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
            evs[0].record(st)
            for i in range(args.steps):
                step(models[m])
                evs[i + 1].record(st)
            torch.cuda.synchronize()
            times[m] += [evs[i].elapsed_time(evs[i + 1]) for i in range(args.steps)]

    # accuracy at B = 2 against the fp32 CPU oracle
    xs = pkg.weights.seeded_pixels(2, 384, 384, seed=2)
    ref = oracle.vision_forward(xs, sd, cfg, False, True)["pooler_output"]
    err = {}
    for m in modes:
        with torch.no_grad():
            got = models[m](pixel_values=xs.cuda(), interpolate_pos_encoding=True).pooler_output.cpu().double()
        d = got - ref.double()
        err[m] = {"max_abs": float(d.abs().max()), "rel_l2": float(d.norm() / ref.double().norm())}

    res = {"metric": "so400m-patch14-384 train fwd+bwd img/s, bf16 vs fp16 compute mode, one process",
           "batch": args.batch, "blocks": args.blocks, "steps_per_block": args.steps}
    for m in modes:
        ms = median(times[m])
        res[m] = {"images_per_sec": round(args.batch / (ms * 1e-3), 2), "ms_per_step_median": round(ms, 2),
                  "ms_per_step_min": round(min(times[m]), 2), "ms_per_step_max": round(max(times[m]), 2),
                  "pooled_err_vs_fp32_oracle_B2": err[m]}
    res["fp16_over_bf16"] = round(res["fp16"]["images_per_sec"] / res["bf16"]["images_per_sec"], 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
