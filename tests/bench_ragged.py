"""What a ragged batch costs next to what the fixed-size entry points can do with the same images: so400m-patch14-384,
bf16 inference, 64 images over 16 distinct sizes x 4 (sides multiples of 14 in 224 .. 518 at 1:1, 4:3 and 16:9, from a
fixed seed).  One process, event-timed, warmed up, medians; the routes alternate in blocks.

Routes:  a  ONE forward_ragged call on the 64 images
         b  64 single-image calls (interpolate_pos_encoding=True)
         c  16 calls, one per size, B = 4 each (the batches stacked beforehand): the best the fixed path can do
         d  the 64 images squashed to 384 x 384, B = 64: for orientation only, it computes something else

Reports ms, images/s and tokens/s per route, and whether (a) equals (b) bit for bit.  No time is fixed in advance.
Prints ONE JSON line; --out writes it.

    python tests/bench_ragged.py [--blocks 2] [--steps 5] [--warmup 2] [--out profiles/ragged_bench.json]
"""
import argparse
import json
import os
import random
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402
from bench_input_grad import median, timed  # noqa: E402

ASPECTS = [(1, 1), (4, 3), (16, 9)]


def draw_sizes(n, P=14, lo=224, hi=518, seed=20):
    """n distinct (H, W), both sides multiples of P in [lo, hi], the long side drawn first, the short one from the aspect."""
    rng = random.Random(seed)
    sizes = []
    while len(sizes) < n:
        a, b = ASPECTS[rng.randrange(len(ASPECTS))]
        long_side = P * rng.randint(lo // P, hi // P)
        short_side = P * round(long_side * b / a / P)
        if short_side < lo:
            continue
        hw = (short_side, long_side) if rng.random() < 0.5 else (long_side, short_side)
        if hw not in sizes:
            sizes.append(hw)
    return sizes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--config", default="so400m-patch14-384")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ragged.py measures on the GPU only"
    pkg = entry.load_package()
    cfg = pkg.get_config(args.config)
    P, S0 = cfg.patch_size, cfg.image_size
    st = torch.cuda.current_stream()
    model = pkg.SiglipVisionModelHIP(cfg, compute_dtype="bf16")
    model.load_state_dict(pkg.weights.seeded_state_dict(cfg, seed=0))
    model = model.cuda().eval().requires_grad_(False)

    sizes = draw_sizes(16, P)
    batches = [pkg.weights.seeded_pixels(4, h, w, seed=100 + i).cuda() for i, (h, w) in enumerate(sizes)]
    singles = [b[j] for b in batches for j in range(4)]                     # 64 views, grouped by size
    ones = [x[None] for x in singles]
    squashed = torch.cat([torch.nn.functional.interpolate(x, size=(S0, S0), mode="bilinear", align_corners=False)
                          for x in ones]).contiguous()
    tokens = sum((x.shape[1] // P) * (x.shape[2] // P) for x in singles)
    n_img = len(singles)

    def ragged():
        return model.forward_ragged(singles)

    def per_image():
        return [model(pixel_values=x, interpolate_pos_encoding=True) for x in ones]

    def per_size():
        return [model(pixel_values=b, interpolate_pos_encoding=True) for b in batches]

    def squash():
        return model(pixel_values=squashed)

    legs = {"a_one_ragged_call": ragged, "b_64_single_image_calls": per_image, "c_16_calls_grouped_by_size": per_size,
            "d_squashed_to_native_B64": squash}
    names = list(legs)
    with torch.no_grad():
        for n in names:
            for _ in range(args.warmup):
                legs[n]()
        torch.cuda.synchronize()
        times = {n: [] for n in names}
        for blk in range(args.blocks):
            for n in (names if blk % 2 == 0 else names[::-1]):
                times[n] += timed(legs[n], args.steps, st)
        a, b = ragged(), per_image()
        torch.cuda.synchronize()
    same = all(torch.equal(a.pooler_output[i].view(torch.int32), o.pooler_output[0].view(torch.int32)) and
               torch.equal(a.unpack(a.last_hidden_state)[i].view(torch.int32), o.last_hidden_state[0].view(torch.int32))
               for i, o in enumerate(b))

    res = {"metric": f"{args.config} bf16 inference, 64 images of 16 sizes: one ragged call against the fixed-size routes; "
                     "one process, event-timed medians, routes alternating in blocks",
           "device": torch.cuda.get_device_name(0), "images": n_img, "sizes_hw": sizes, "tokens_T": tokens,
           "tokens_squashed": n_img * (S0 // P) ** 2, "blocks": args.blocks, "steps_per_block": args.steps,
           "warmup": args.warmup, "a_equals_b_bitwise": bool(same), "routes": {}}
    for n in names:
        t = times[n]
        ms = median(t)
        toks = n_img * (S0 // P) ** 2 if n.startswith("d_") else tokens
        res["routes"][n] = {"ms_median": round(ms, 3), "ms_min": round(min(t), 3), "ms_max": round(max(t), 3),
                            "samples": len(t), "images_per_s": round(n_img / ms * 1e3, 1),
                            "tokens_per_s": round(toks / ms * 1e3)}
    r = res["routes"]
    res["b_over_a"] = round(r["b_64_single_image_calls"]["ms_median"] / r["a_one_ragged_call"]["ms_median"], 3)
    res["c_over_a"] = round(r["c_16_calls_grouped_by_size"]["ms_median"] / r["a_one_ragged_call"]["ms_median"], 3)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
