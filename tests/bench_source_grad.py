"""What the gradient with respect to SOURCE-resolution images costs on top of d loss / d pixel_values: so400m-patch14-384,
bf16, B = 128, frozen encoder, one process, alternating event-timed blocks (the method of tests/bench_input_grad.py).

Legs:  pixels   the attack step from a (B,3,384,384) pixel tensor (bench_input_grad.py's leg b: the baseline, re-timed here)
       source   the attack step from (B,3,1024,1024) float sources through the differentiable preprocess.resize_normalize
and, alone, on buffers of the step's shapes: the transform's forward (sgl_op_preprocess) and its backward
(sgl_op_preprocess_bwd, pre-pass included), the latter with GB/s over the bytes that must move: d_out read once, d_src
written once.

One condition follows from the launch lists and is recorded as a boolean: source - pixels is what the forward and the
backward take alone, within the spread of the step times.  Prints ONE JSON line; --out also writes it to a file.

    python tests/bench_source_grad.py [--batch 128] [--source 1024] [--blocks 4] [--steps 4] [--warmup 2] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402
from bench_input_grad import median, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--source", type=int, default=1024)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    pkg = entry.load_package()
    lib = pkg.lib.load()
    pp = pkg.preprocess
    cfg = pkg.get_config("so400m-patch14-384")
    B, S, Hs = args.batch, 384, args.source
    model = pkg.SiglipVisionModelHIP(cfg, compute_dtype="bf16")
    model.load_state_dict(pkg.weights.seeded_state_dict(cfg, seed=0))
    model = model.cuda().requires_grad_(False)
    gen = torch.Generator(device="cuda").manual_seed(1)
    src = torch.rand(B, 3, Hs, Hs, device="cuda", generator=gen)
    srcg = src.clone().requires_grad_(True)
    xg = pp.resize_normalize(src, S).requires_grad_(True)
    st = torch.cuda.current_stream()

    def step(pixels, leaf):
        out = model(pixel_values=pixels, interpolate_pos_encoding=True)
        out.pooler_output.square().mean().backward()
        leaf.grad = None

    legs = {"pixels_attack_step": lambda: step(xg, xg), "source_attack_step": lambda: step(pp.resize_normalize(srcg, S), srcg)}
    names = list(legs)
    for n in names:
        for _ in range(args.warmup):
            legs[n]()
    torch.cuda.synchronize()
    times = {n: [] for n in names}
    for blk in range(args.blocks):
        for n in (names if blk % 2 == 0 else names[::-1]):
            times[n] += timed(legs[n], args.steps, st)

    # the two added launches alone
    s = pkg.lib.current_stream_handle(src.device)
    out = torch.empty(B, 3, S, S, device="cuda")
    g = torch.randn(B, 3, S, S, device="cuda", generator=gen)
    dsrc = torch.empty(B, 3, Hs, Hs, device="cuda")
    nbytes = lib.sgl_op_preprocess_bwd_scratch_bytes(B, Hs, Hs, S)
    scratch = torch.empty(max(nbytes, 1), device="cuda", dtype=torch.uint8)

    def fwd():
        assert lib.sgl_op_preprocess(src.data_ptr(), 0, B, Hs, Hs, out.data_ptr(), pkg.lib.SGL_DTYPE_F32, S, 14, 640, 0, 0.5, 0.5,
                                     None, 1.0, s) == 0

    def bwd():
        assert lib.sgl_op_preprocess_bwd(g.data_ptr(), B, Hs, Hs, S, 0.5, None, 1.0, dsrc.data_ptr(), scratch.data_ptr(),
                                         nbytes, s) == 0

    alone = {}
    for name, fn in (("transform_forward", fwd), ("transform_backward", bwd)):
        for _ in range(3):
            fn()
        t = timed(fn, 20, st)
        alone[name] = {"ms_median": round(median(t), 4), "ms_min": round(min(t), 4), "ms_max": round(max(t), 4)}
    moved = {"transform_forward": src.numel() * 4 + out.numel() * 4, "transform_backward": g.numel() * 4 + dsrc.numel() * 4}
    for k, nb in moved.items():
        alone[k]["bytes_moved"] = nb
        alone[k]["GB_per_s"] = round(nb / (alone[k]["ms_median"] * 1e-3) / 1e9, 1)

    res = {"metric": "so400m-patch14-384 bf16, frozen encoder: cost of d loss / d source images through the differentiable "
                     "input transform, one process, alternating blocks",
           "batch": B, "source_hw": [Hs, Hs], "blocks": args.blocks, "steps_per_block": args.steps,
           "device": torch.cuda.get_device_name(0)}
    for n in names:
        ms = median(times[n])
        res[n] = {"ms_per_step_median": round(ms, 2), "ms_per_step_min": round(min(times[n]), 2),
                  "ms_per_step_max": round(max(times[n]), 2), "images_per_sec": round(B / (ms * 1e-3), 2)}
    res["added_launches_alone"] = alone
    a, b = (res[k]["ms_per_step_median"] for k in names)
    explained = alone["transform_forward"]["ms_median"] + alone["transform_backward"]["ms_median"]
    spread = max(res[k]["ms_per_step_max"] - res[k]["ms_per_step_min"] for k in names)
    res["source_minus_pixels_ms"] = round(b - a, 3)
    res["explained_by_added_launches_ms"] = round(explained, 3)
    res["step_time_spread_ms"] = round(spread, 3)
    res["condition_added_time_explained"] = bool(abs((b - a) - explained) <= spread)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
