"""Block recompute (gradient checkpointing) vs the default activation policy, one process.

Leg 1: so400m-patch14-384, bf16, training forward + backward at B = 128, recompute off and on, timed in alternating
blocks of event-timed steps after a warm-up (the step bench.py times: forward, mean-square pooled loss, backward, every
shadow re-cast).  Per policy: median img/s, the peak of torch.cuda.max_memory_allocated over one step, and the bytes
held from forward to backward (memory_allocated after the forward minus before it, outputs excluded: saved + hidden
states), plus the shared block region a recompute context keeps in its workspace.
Leg 2: google/siglip2-so400m-patch16-512 at B = 256 with recompute (the default policy's footprint at that batch is
reported; it does not fit).
Before each leg the footprint predicted from the size query is compared with torch.cuda.mem_get_info(); a leg that
would not fit is skipped and the output says so.  Prints ONE JSON line.

    python tests/bench_recompute.py [--batch 128] [--batch512 256] [--blocks 4] [--steps 5] [--warmup 3]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402

GB = 1e9


def median(v):
    v = sorted(v)
    n = len(v)
    return v[n // 2] if n % 2 else 0.5 * (v[n // 2 - 1] + v[n // 2])


def predicted_bytes(model, B, res, recompute):
    """Device memory of one training step: fp32 masters + gradients, shadow, saved, workspace, the L+1 hidden states,
    last_hidden_state and its gradient, pooled, the input."""
    cfg = model.config
    L, D, N = cfg.num_hidden_layers, cfg.hidden_size, (res // cfg.patch_size) ** 2
    sh, saved, ws = model._contexts.sizes(B, res, res, True, recompute)
    nparam = sum(p.numel() for p in model.parameters())
    return 8 * nparam + sh + saved + ws + (L + 3) * B * N * D * 4 + B * D * 4 + B * 3 * res * res * 4, saved, ws


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--batch512", type=int, default=256)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    pkg = entry.load_package()
    pkg.lib.load()
    st = torch.cuda.current_stream()
    res = {"metric": "train fwd+bwd img/s and memory, block recompute vs default policy, bf16, one process"}

    def step(model, x):
        params = list(model.parameters())
        torch.autograd.graph.increment_version(params)   # as bench.py: every shadow is re-cast each step
        out = model(pixel_values=x, interpolate_pos_encoding=True)
        out.pooler_output.square().mean().backward()
        for p in params:
            p.grad = None

    def memory(model, x):
        """(peak bytes of one step over what was resident before it, bytes held from forward to backward)."""
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = model(pixel_values=x, interpolate_pos_encoding=True)
        torch.cuda.synchronize()
        held = torch.cuda.memory_allocated() - base - out.last_hidden_state.numel() * 4 - out.pooler_output.numel() * 4
        out.pooler_output.square().mean().backward()
        del out
        for p in model.parameters():
            p.grad = None
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base, torch.cuda.max_memory_allocated(), held

    # ---- leg 1: so400m@384, B = 128, both policies
    cfg = pkg.get_config("so400m-patch14-384")
    sd = pkg.weights.seeded_state_dict(cfg, seed=0)
    B = args.batch
    policies = (False, True)
    models, leg = {}, {}
    for rc in policies:
        model = pkg.SiglipVisionModelHIP(cfg, compute_dtype="bf16", recompute=rc)
        model.load_state_dict(sd)
        models[rc] = model.cuda()
    x = pkg.weights.seeded_pixels(B, 384, 384, seed=1).cuda()
    free = torch.cuda.mem_get_info()[0]
    run = {}
    for rc in policies:
        need, saved, ws = predicted_bytes(models[rc], B, 384, rc)
        name = "recompute" if rc else "none"
        run[rc] = need <= 0.95 * free      # both models' parameters are resident already: a conservative check
        leg[name] = {"predicted_step_bytes": need, "saved_bytes": saved, "ws_bytes": ws}
        if not run[rc]:
            leg[name]["skipped"] = f"predicted {need / GB:.1f} GB > free {free / GB:.1f} GB"
    for rc in policies:
        if run[rc]:
            for _ in range(args.warmup):
                step(models[rc], x)
    torch.cuda.synchronize()
    times = {rc: [] for rc in policies}
    for blk in range(args.blocks):
        for rc in (policies if blk % 2 == 0 else policies[::-1]):
            if not run[rc]:
                continue
            evs = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
            evs[0].record(st)
            for i in range(args.steps):
                step(models[rc], x)
                evs[i + 1].record(st)
            torch.cuda.synchronize()
            times[rc] += [evs[i].elapsed_time(evs[i + 1]) for i in range(args.steps)]
    region = models[True]._contexts.sizes(B, 384, 384, True, True)[2] - models[False]._contexts.sizes(B, 384, 384, True, False)[2]
    for rc in policies:
        if not run[rc]:
            continue
        name = "recompute" if rc else "none"
        ms = median(times[rc])
        peak_step, peak_abs, held = memory(models[rc], x)
        leg[name].update({"images_per_sec": round(B / (ms * 1e-3), 2), "ms_per_step_median": round(ms, 2),
                          "ms_per_step_min": round(min(times[rc]), 2), "ms_per_step_max": round(max(times[rc]), 2),
                          "timed_steps": len(times[rc]), "step_peak_bytes_over_resident": peak_step,
                          "max_memory_allocated": peak_abs, "held_fwd_to_bwd_bytes": held})
        if rc:
            leg[name]["shared_block_region_bytes"] = region
    if run[False] and run[True]:
        leg["recompute_over_none_img_s"] = round(leg["recompute"]["images_per_sec"] / leg["none"]["images_per_sec"], 4)
        leg["recompute_over_none_held"] = round(
            (leg["recompute"]["held_fwd_to_bwd_bytes"] + region) / leg["none"]["held_fwd_to_bwd_bytes"], 4)
    res["so400m-patch14-384_B%d" % B] = leg
    del models, x
    torch.cuda.empty_cache()

    # ---- leg 2: so400m-patch16-512, B = 256, recompute only
    cfg = pkg.get_config("google/siglip2-so400m-patch16-512")
    B2 = args.batch512
    model = pkg.SiglipVisionModelHIP(cfg, compute_dtype="bf16", recompute=True)
    model.load_state_dict(pkg.weights.seeded_state_dict(cfg, seed=0))
    model = model.cuda()
    free = torch.cuda.mem_get_info()[0]
    need_none = predicted_bytes(model, B2, 512, False)[0]
    need, saved, ws = predicted_bytes(model, B2, 512, True)
    leg = {"predicted_step_bytes": need, "saved_bytes": saved, "ws_bytes": ws, "free_bytes": free,
           "none_predicted_step_bytes": need_none,
           "none": f"not run: predicted {need_none / GB:.1f} GB vs {free / GB:.1f} GB free"
           if need_none > 0.95 * free else "fits but not run"}
    if need <= 0.95 * free:
        x = pkg.weights.seeded_pixels(B2, 512, 512, seed=1).cuda()
        for _ in range(args.warmup):
            step(model, x)
        torch.cuda.synchronize()
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(2 * args.steps + 1)]
        evs[0].record(st)
        for i in range(2 * args.steps):
            step(model, x)
            evs[i + 1].record(st)
        torch.cuda.synchronize()
        t = [evs[i].elapsed_time(evs[i + 1]) for i in range(2 * args.steps)]
        peak_step, peak_abs, held = memory(model, x)
        leg.update({"images_per_sec": round(B2 / (median(t) * 1e-3), 2), "ms_per_step_median": round(median(t), 2),
                    "timed_steps": len(t), "step_peak_bytes_over_resident": peak_step,
                    "max_memory_allocated": peak_abs, "held_fwd_to_bwd_bytes": held})
    else:
        leg["skipped"] = f"predicted {need / GB:.1f} GB > free {free / GB:.1f} GB"
    res["so400m-patch16-512_B%d_recompute" % B2] = leg
    print(json.dumps(res))


if __name__ == "__main__":
    main()
