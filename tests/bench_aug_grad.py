"""What the gradient of the video trainer's augmenting input transform with respect to its source costs: a float source
B = 128, 224 x 224 -> S = 384, draws of `preprocess.sample_augmentation` with a fixed seed.  One process, event-timed,
warm-up calls first, medians, the routes alternating in blocks (the method of tests/bench_views_grad.py).

Legs (forward + `backward` of one fixed grad_out each, same shapes):
    aug  `preprocess.augment_resize_normalize(differentiable=True)`: sgl_op_preprocess_aug + sgl_op_preprocess_aug_bwd
    a    `preprocess.resize_normalize`, the plain differentiable branch (no augmentation): what the linear part costs
    b    the fp32 restatement of tests/aug_bwd_ref.py built from torch operators on the device under autograd: the only
         route to this gradient without sgl_op_preprocess_aug_bwd
    bwd  the sgl_op_preprocess_aug_bwd call alone on preallocated buffers, and its share of the 225 ms attack step
         (so400m@384, B = 128, frozen bf16 encoder: README)

The gradients of `aug` and `b` are compared on the pixels the restatement does not flag as near a kink (max|e| / max|ref|
and relative L2 over the batch, b as the reference: both are fp32).  No time is fixed in advance.  Prints ONE JSON line;
--out writes it.

    python tests/bench_aug_grad.py [--blocks 4] [--steps 5] [--warmup 3] [--out profiles/aug_grad_bench.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__ as entry  # noqa: E402
import aug_bwd_ref as ar  # noqa: E402
from bench_input_grad import median, timed  # noqa: E402
from bench_views_grad import stats  # noqa: E402

ATTACK_STEP_MS = 225.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--source", type=int, default=224)
    ap.add_argument("--size", type=int, default=384)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_aug_grad.py measures on the GPU only"
    assert args.blocks * args.steps >= 20, "medians of at least 20"
    pkg = entry.load_package()
    lib = pkg.lib.load()
    pp = pkg.preprocess
    dev = torch.device("cuda")
    st = torch.cuda.current_stream()
    B, Hs, S = args.batch, args.source, args.size
    recs = pp.sample_augmentation(B, torch.Generator().manual_seed(1))
    for r in recs:                                        # the fp32 values the device table holds, for both routes
        for k in ("cos", "sin", "brightness", "contrast", "saturation", "hue"):
            r[k] = ar._f32c(r[k])
    src = torch.rand(B, 3, Hs, Hs, generator=torch.Generator().manual_seed(2)).to(dev)
    G = torch.randn(B, 3, S, S, generator=torch.Generator().manual_seed(3)).to(dev)
    xg = src.clone().requires_grad_(True)
    grads = {}

    def route(name, fwd):
        def run():
            xg.grad = None
            fwd(xg).backward(G)
            grads[name] = xg.grad
        return run

    legs = {"aug_differentiable": route("aug", lambda x: pp.augment_resize_normalize(x, S, recs, differentiable=True)),
            "a_resize_normalize": route("a", lambda x: pp.resize_normalize(x, S)),
            "b_torch_restatement_fp32": route("b", lambda x: ar.forward(x, S, recs)[0])}
    names = list(legs)
    for n in names:
        for _ in range(args.warmup):
            legs[n]()
    torch.cuda.synchronize()
    times = {n: [] for n in names}
    for blk in range(args.blocks):
        for n in (names if blk % 2 == 0 else names[::-1]):
            times[n] += timed(legs[n], args.steps, st)
    res = {"metric": f"forward + backward to a {B}x3x{Hs}x{Hs} float source through the augmenting transform at S = {S} "
                     "(draws of sample_augmentation, seed 1), against the plain differentiable branch and the per-operator "
                     "torch route; one process, event-timed medians, the routes alternating in blocks",
           "batch": B, "source_hw": [Hs, Hs], "size": S, "blocks": args.blocks, "steps_per_block": args.steps,
           "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
           "records": {"flipped": sum(r["flip"] for r in recs), "rotated": sum(r["sin"] != 0.0 for r in recs),
                       "jittered": sum(r["order"] is not None for r in recs)}}
    for n in names:
        res[n] = stats(times[n])
    t_aug, t_a, t_b = (res[n]["ms_median"] for n in names)
    res["aug_over_a"] = round(t_aug / t_a, 3)
    res["b_over_aug"] = round(t_b / t_aug, 2)

    with torch.no_grad():
        keep = (~ar.forward(src, S, recs)[1])[:, None]
    y = pp.augment_resize_normalize(xg, S, recs, differentiable=True)
    xg.grad = None
    y.backward(G * keep)
    g_aug = xg.grad.double()
    xg.grad = None
    ar.forward(xg, S, recs)[0].backward(G * keep)
    g_b = xg.grad.double()
    e = g_aug - g_b
    res["aug_vs_b_on_unflagged_pixels"] = {"flagged_share": round(1.0 - keep.double().mean().item(), 5),
                                           "max_err_over_max_ref": float(f"{(e.abs().max() / g_b.abs().max()).item():.3e}"),
                                           "rel_l2": float(f"{(e.norm() / g_b.norm()).item():.3e}")}

    tab = pp.augment_table(recs, dev)
    nbytes = lib.sgl_op_preprocess_aug_bwd_scratch_bytes(B, Hs, Hs, S)
    scratch = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    d_src = torch.empty(B, 3, Hs, Hs, device=dev, dtype=torch.float32)
    s = pkg.lib.current_stream_handle(dev)

    def launch():
        assert lib.sgl_op_preprocess_aug_bwd(G.data_ptr(), src.data_ptr(), 0, B, Hs, Hs, S, 0.5, tab.data_ptr(),
                                             d_src.data_ptr(), scratch.data_ptr(), nbytes, s) == 0
    for _ in range(args.warmup):
        launch()
    t = timed(launch, args.blocks * args.steps, st)
    xg.grad = None
    pp.augment_resize_normalize(xg, S, recs, differentiable=True).backward(G)
    res["bwd_call_alone"] = dict(stats(t), scratch_bytes=nbytes, equals_autograd_bitwise=bool(torch.equal(d_src, xg.grad)),
                                 share_of_the_225_ms_attack_step=round(median(t) / ATTACK_STEP_MS, 4))
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
