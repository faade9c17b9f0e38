"""What the gradient of the app's test-time views with respect to the source image costs: one 1 x 3 x 1024 x 1024 float
source, the 42 views of `preprocess.detect_views`, S = 384.  One process, event-timed, 3 warm-up calls, medians of 25, the
two routes alternating in blocks (the method of tests/bench_views.py).

Legs:  a  what there was before sgl_op_preprocess_views_bwd: the per-view torch composition (slice, `rot90` or an index
          gather for the kept canvas, flip, `preprocess.resize_normalize` per view, `cat`), forward + `backward` of a fixed
          grad_out: 42 forward launches, 42 backward launches, autograd's full-frame adds
       b  `preprocess.views_resize_normalize(differentiable=True)`, forward + `backward` of the same grad_out
       c  the `sgl_op_preprocess_views_bwd` call alone on preallocated buffers (pre-pass + gather), its algorithmic bytes
          (d_out read once, d_src written once, the tables written and read once) and the GB/s that makes
       d  the whole attack step on the 42 rows: so400m-patch14-384, bf16, frozen encoder, forward + backward to the source
          through route b, and route b's share of it

The two routes' gradients must agree within the sum of their bounds (tests/views_bwd_ref.py; torch's per-view route adds
the same terms in another order, so the same bound holds for it).  No time is fixed in advance; whether b <= a is
recorded as it comes out.  Prints ONE JSON line; --out writes it.

    python tests/bench_views_grad.py [--blocks 5] [--steps 5] [--warmup 3] [--out profiles/views_grad_bench.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__ as entry  # noqa: E402
import views_bwd_ref as vb  # noqa: E402
import views_ref as vr  # noqa: E402
from bench_input_grad import median, timed  # noqa: E402


def stats(t, nd=4):
    return {"ms_median": round(median(t), nd), "ms_min": round(min(t), nd), "ms_max": round(max(t), nd), "calls": len(t)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--side", type=int, default=1024)
    ap.add_argument("--config", default="so400m-patch14-384")
    ap.add_argument("--no-attack", action="store_true", help="skip leg d (the full encoder)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_views_grad.py measures on the GPU only"
    pkg = entry.load_package()
    lib = pkg.lib.load()
    pp = pkg.preprocess
    cfg = pkg.get_config(args.config)
    S = cfg.image_size
    dev = torch.device("cuda")
    st = torch.cuda.current_stream()
    s = pkg.lib.current_stream_handle(dev)
    h = w = args.side
    d = pp.detect_views(h, w)
    views = d.views
    V = len(views)
    src = torch.rand(1, 3, h, w, generator=torch.Generator().manual_seed(1)).to(dev)
    G_cpu = vb.grad_input(V, S, seed=2)
    G = G_cpu.to(dev)
    xg = src.clone().requires_grad_(True)

    canvas = {}                                           # the kept-canvas gathers' index tensors, built outside the timing
    for v in views:
        if v.turns and v.keep_canvas:
            x0, y0, x1, y1 = v.box
            cy, cx, inside = vr.keep_canvas_index(y1 - y0, x1 - x0, v.turns)
            canvas[(y1 - y0, x1 - x0, v.turns)] = (cy.to(dev), cx.to(dev), inside.to(dev))

    def per_view(x):
        rows = []
        for v in views:
            x0, y0, x1, y1 = v.box
            c = x[v.src:v.src + 1, :, y0:y1, x0:x1]
            if v.turns and v.keep_canvas:
                cy, cx, inside = canvas[(y1 - y0, x1 - x0, v.turns)]
                c = torch.where(inside, c[..., cy, cx], c.new_zeros(()))
            elif v.turns:
                c = torch.rot90(c, v.turns, dims=(-2, -1))
            if v.flip:
                c = c.flip(-1)
            rows.append(pp.resize_normalize(c, S))
        return torch.cat(rows)

    grads = {}

    def route(name, fwd):
        def run():
            xg.grad = None
            fwd(xg).backward(G)
            grads[name] = xg.grad
        return run

    legs = {"a_per_view_torch_route": route("a", per_view),
            "b_views_differentiable": route("b", lambda x: pp.views_resize_normalize(x, views, S, differentiable=True))}
    names = list(legs)
    for n in names:
        for _ in range(args.warmup):
            legs[n]()
    torch.cuda.synchronize()
    times = {n: [] for n in names}
    for blk in range(args.blocks):
        for n in (names if blk % 2 == 0 else names[::-1]):
            times[n] += timed(legs[n], args.steps, st)
    res = {"metric": f"gradient of the app's {V} test-time views with respect to one 1x3x{h}x{w} float source at S = {S}: "
                     "forward + backward of a fixed grad_out, per-view torch route against the one-pass route; one "
                     "process, event-timed medians, the routes alternating in blocks",
           "views": V, "size": S, "source_hw": [h, w], "blocks": args.blocks, "steps_per_block": args.steps,
           "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
    for n in names:
        res[n] = stats(times[n])
    a, b = res[names[0]]["ms_median"], res[names[1]]["ms_median"]
    res["a_over_b"] = round(a / b, 3)
    res["b_not_slower_than_a"] = bool(b <= a)

    torch.set_num_threads(min(16, torch.get_num_threads()))
    ref, bound, _ = vb.views_bwd_ref(G_cpu, [vr.as_tuple(v) for v in views], 1, h, w, S, 0.5)
    ga, gb = grads["a"].cpu().double(), grads["b"].cpu().double()
    res["gradients_agree_within_the_sum_of_bounds"] = bool(((ga - gb).abs() <= 2 * bound).all())
    res["worst_err_over_bound"] = {"a": round(((ga - ref).abs() / bound).max().item(), 4),
                                   "b": round(((gb - ref).abs() / bound).max().item(), 4)}

    tab = pp.view_table(views, 1, h, w)
    nbytes = lib.sgl_op_preprocess_views_bwd_scratch_bytes(tab, V, S)
    scratch = torch.empty(max(nbytes, 1), device=dev, dtype=torch.uint8)
    d_src = torch.empty(1, 3, h, w, device=dev, dtype=torch.float32)

    def launch():
        assert lib.sgl_op_preprocess_views_bwd(G.data_ptr(), 1, h, w, tab, V, S, 0.5, d_src.data_ptr(), scratch.data_ptr(),
                                               nbytes, s) == 0
    for _ in range(args.warmup):
        launch()
    t = timed(launch, args.blocks * args.steps, st)
    moved = G.numel() * 4 + d_src.numel() * 4 + 2 * nbytes
    res["c_views_bwd_call_alone"] = dict(stats(t), scratch_bytes=nbytes, algorithmic_bytes=moved,
                                         GB_per_s=round(moved / (median(t) * 1e-3) / 1e9, 1),
                                         equals_route_b_bitwise=bool(torch.equal(d_src, grads["b"])))

    if not args.no_attack:
        model = pkg.SiglipVisionModelHIP(cfg, compute_dtype="bf16")
        model.load_state_dict(pkg.weights.seeded_state_dict(cfg, seed=0))
        model = model.cuda().eval().requires_grad_(False)
        wgt = torch.cos(torch.arange(V * cfg.hidden_size, dtype=torch.float32, device=dev) * 0.37).view(V, -1)

        def attack():
            xg.grad = None
            px = pp.views_resize_normalize(xg, views, S, differentiable=True)
            (model(pixel_values=px).pooler_output.float() * wgt).sum().backward()
        for _ in range(args.warmup):
            attack()
        t = timed(attack, args.blocks * args.steps, st)
        res["d_attack_step_42_rows_frozen_bf16"] = dict(stats(t, 3), views_fwd_bwd_share=round(b / median(t), 4))
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
