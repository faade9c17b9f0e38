"""What d loss / d pixel_values costs: so400m-patch14-384, bf16, B = 128, one process, alternating event-timed blocks
(the method of tests/bench_fp16.py).

Legs:  a  no_grad forward
       b  frozen encoder, forward + backward to d_pixels (the attack / saliency step)
       c  the full training step bench.py times (every parameter trains, every shadow re-cast)
       d  c + d_pixels
       e  b with recompute=True
and, alone, the three launches the pixel gradient adds to a backward: the W_patch^T cast-transpose, the dX GEMM
(2 * M * Kp * D flop) and col2im (GB/s over the bytes it has to move: the 3*P*P used columns in, every pixel out).

Two conditions follow from the launch lists and are recorded as booleans: b takes less time than c (it is c's launches
minus every dW GEMM and bias reduction, plus the three above), and d - c is what the three launches take alone, within the
spread of the step times.  Prints ONE JSON line; --out also writes it to a file.

    python tests/bench_input_grad.py [--batch 128] [--blocks 4] [--steps 4] [--warmup 2] [--out FILE]
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


def timed(fn, n, st):
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
    evs[0].record(st)
    for i in range(n):
        fn()
        evs[i + 1].record(st)
    torch.cuda.synchronize()
    return [evs[i].elapsed_time(evs[i + 1]) for i in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    pkg = entry.load_package()
    lib = pkg.lib.load()
    cfg = pkg.get_config("so400m-patch14-384")
    sd = pkg.weights.seeded_state_dict(cfg, seed=0)
    B, S, P, D = args.batch, 384, cfg.patch_size, cfg.hidden_size

    def make(frozen, recompute):
        m = pkg.SiglipVisionModelHIP(cfg, compute_dtype="bf16", recompute=recompute)
        m.load_state_dict(sd)
        m = m.cuda()
        if frozen:
            m.requires_grad_(False)
        return m

    trainable, frozen, frozen_rc = make(False, False), make(True, False), make(True, True)
    x = pkg.weights.seeded_pixels(B, S, S, seed=1).cuda()
    xg = x.clone().requires_grad_(True)
    st = torch.cuda.current_stream()

    def leg_a():
        with torch.no_grad():
            frozen(pixel_values=x, interpolate_pos_encoding=True)

    def attack(model):
        out = model(pixel_values=xg, interpolate_pos_encoding=True)
        out.pooler_output.square().mean().backward()
        xg.grad = None

    def train(inp):
        params = list(trainable.parameters())
        torch.autograd.graph.increment_version(params)   # as bench.py: every shadow is re-cast each step
        out = trainable(pixel_values=inp, interpolate_pos_encoding=True)
        out.pooler_output.square().mean().backward()
        for p in params:
            p.grad = None
        xg.grad = None

    legs = {"a_no_grad_forward": leg_a, "b_frozen_d_pixels": lambda: attack(frozen), "c_train_step": lambda: train(x),
            "d_train_step_d_pixels": lambda: train(xg), "e_frozen_d_pixels_recompute": lambda: attack(frozen_rc)}
    names = list(legs)
    for n in names:
        for _ in range(args.warmup):
            legs[n]()
    torch.cuda.synchronize()
    times = {n: [] for n in names}
    for blk in range(args.blocks):
        for n in (names if blk % 2 == 0 else names[::-1]):
            times[n] += timed(legs[n], args.steps, st)

    # the three added launches alone, on buffers of the step's shapes
    gh = S // P
    M, K0 = B * gh * gh, 3 * P * P
    Kp = (K0 + 63) // 64 * 64
    s = pkg.lib.current_stream_handle(x.device)
    g = torch.randn(M, D, device="cuda").bfloat16()
    wpt = torch.randn(Kp, D, device="cuda").bfloat16()
    dcols = torch.empty(M, Kp, device="cuda")
    dpix = torch.empty(B, 3, S, S, device="cuda")
    wmaster = torch.randn(D, K0, device="cuda")

    def gemm():
        assert lib.sgl_op_gemm_nt(pkg.lib.SGL_DTYPE_BF16, g.data_ptr(), D, wpt.data_ptr(), D, M, Kp, D, pkg.lib.EPI_F32,
                                  dcols.data_ptr(), Kp, None, 0, None, None, 0, None, 0, None, 0, 0, 0, 0, 0, 0, s) == 0

    def col2im(cl=0):
        assert lib.sgl_op_col2im(dcols.data_ptr(), B, S, S, P, Kp, dpix.data_ptr(), cl, s) == 0

    def cast_t():   # PROXY: a torch transposed copy of the same bytes; the library's cast_job launch has no entry of its own
        wpt[:K0].copy_(wmaster.t())

    alone = {}
    for name, fn in (("dx_gemm", gemm), ("col2im_nchw", col2im), ("col2im_nhwc", lambda: col2im(1)),
                     ("wpatch_t_cast", cast_t)):
        for _ in range(3):
            fn()
        t = timed(fn, 20, st)
        alone[name] = {"ms_median": round(median(t), 4), "ms_min": round(min(t), 4), "ms_max": round(max(t), 4)}
    c2i_bytes = M * K0 * 4 + B * 3 * S * S * 4
    for k in ("col2im_nchw", "col2im_nhwc"):
        alone[k]["bytes_moved"] = c2i_bytes
        alone[k]["GB_per_s"] = round(c2i_bytes / (alone[k]["ms_median"] * 1e-3) / 1e9, 1)
    alone["wpatch_t_cast"]["note"] = "proxy: torch copy_ of the transposed 1152x588 matrix, not the cast_job launch itself"
    alone["dx_gemm"]["flop"] = 2 * M * Kp * D
    alone["dx_gemm"]["TFLOP_per_s"] = round(2 * M * Kp * D / (alone["dx_gemm"]["ms_median"] * 1e-3) / 1e12, 1)

    res = {"metric": "so400m-patch14-384 bf16: cost of d loss / d pixel_values, one process, alternating blocks",
           "batch": B, "blocks": args.blocks, "steps_per_block": args.steps, "device": torch.cuda.get_device_name(0)}
    for n in names:
        ms = median(times[n])
        res[n] = {"ms_per_step_median": round(ms, 2), "ms_per_step_min": round(min(times[n]), 2),
                  "ms_per_step_max": round(max(times[n]), 2), "images_per_sec": round(B / (ms * 1e-3), 2)}
    res["added_launches_alone"] = alone
    b, c, d = (res[k]["ms_per_step_median"] for k in ("b_frozen_d_pixels", "c_train_step", "d_train_step_d_pixels"))
    explained = alone["dx_gemm"]["ms_median"] + alone["col2im_nchw"]["ms_median"] + alone["wpatch_t_cast"]["ms_median"]
    spread = max(res[k]["ms_per_step_max"] - res[k]["ms_per_step_min"] for k in ("c_train_step", "d_train_step_d_pixels"))
    res["d_minus_c_ms"] = round(d - c, 3)
    res["explained_by_added_launches_ms"] = round(explained, 3)
    res["step_time_spread_ms"] = round(spread, 3)
    res["condition_b_faster_than_c"] = bool(b < c)
    res["condition_d_minus_c_explained"] = bool(abs((d - c) - explained) <= spread)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
