"""bf16 vs mxfp8 compute mode, same process: no_grad forward throughput and the NT GEMMs of the encoder.

Both encoders live in one process and are timed in alternating blocks of event-timed forwards after a warm-up, so that
clock drift (DVFS) and allocator state hit both modes alike.  Prints ONE JSON line:
  * so400m-patch14-384 forward img/s at B = 9, 64, 256 and base-patch16-224 at B = 512, per mode (median of the
    per-forward times), and the mxfp8 / bf16 ratio;
  * per-shape NT GEMM TF/s at M = 186 624 (so400m@384 B = 256), bf16 kernel (sgl_op_gemm_nt) against the MX kernel
    (sgl_op_gemm_nt_mx), with the encoder's epilogues (QKV scatter, residual add, GELU);
  * each mode's pooled-output error against the fp32 oracle at B = 2 (so400m@384, seeded weights).

    python tests/bench_mxfp8.py [--blocks 4] [--steps 5] [--warmup 3]
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


def alternate(fns, blocks, steps, warmup):
    """{name: [ms per call]} for the callables in fns, timed in alternating blocks."""
    st = torch.cuda.current_stream()
    for f in fns.values():
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    names = list(fns)
    times = {n: [] for n in names}
    for blk in range(blocks):
        for n in (names if blk % 2 == 0 else names[::-1]):
            evs = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
            evs[0].record(st)
            for i in range(steps):
                fns[n]()
                evs[i + 1].record(st)
            torch.cuda.synchronize()
            times[n] += [evs[i].elapsed_time(evs[i + 1]) for i in range(steps)]
    return times


def forward_bench(pkg, name, res, batch, args):
    cfg = pkg.get_config(name)
    sd = pkg.weights.seeded_state_dict(cfg, seed=0)
    models = {}
    for m in ("bf16", "mxfp8"):
        model = pkg.SiglipVisionModelHIP(cfg, compute_dtype=m)
        model.load_state_dict(sd)
        models[m] = model.cuda()
    x = pkg.weights.seeded_pixels(batch, res, res, seed=1).cuda()

    def fwd(model):
        def f():
            with torch.no_grad():
                model(pixel_values=x, interpolate_pos_encoding=True)
        return f

    times = alternate({m: fwd(models[m]) for m in models}, args.blocks, args.steps, args.warmup)
    out = {}
    for m, t in times.items():
        ms = median(t)
        out[m] = {"images_per_sec": round(batch / (ms * 1e-3), 1), "ms_median": round(ms, 3),
                  "ms_min": round(min(t), 3), "ms_max": round(max(t), 3)}
    out["mxfp8_over_bf16"] = round(out["mxfp8"]["images_per_sec"] / out["bf16"]["images_per_sec"], 4)
    del models
    torch.cuda.empty_cache()
    return out


def gemm_bench(pkg, M, N, K, args):
    lib = pkg.lib.load()
    s = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda").manual_seed(N + K)
    A = torch.randn(M, K, device="cuda", generator=g).bfloat16()
    B = (torch.randn(N, K, device="cuda", generator=g) / K ** 0.5).bfloat16()
    bias = torch.zeros(N, device="cuda")
    Kp = (K + 127) // 128 * 128
    Aq = torch.empty(M, Kp, dtype=torch.uint8, device="cuda")
    As = torch.empty(M, Kp // 32, dtype=torch.uint8, device="cuda")
    Bq = torch.empty(N, Kp, dtype=torch.uint8, device="cuda")
    Bs = torch.empty(N, Kp // 32, dtype=torch.uint8, device="cuda")
    pkg.lib.check(lib.sgl_op_quantize_mxfp8(A.data_ptr(), 1, K, M, K, Kp, Aq.data_ptr(), As.data_ptr(), s), "quantize")
    pkg.lib.check(lib.sgl_op_quantize_mxfp8(B.data_ptr(), 1, K, N, K, Kp, Bq.data_ptr(), Bs.data_ptr(), s), "quantize")
    if N == 3 * 1152:   # QKV: head-major bf16 scatter
        epi, heads, hd, hdp, tokens = pkg.lib.EPI_QKV, 16, 72, 80, 729
        out = torch.empty(3 * M * 16 * 80, dtype=torch.bfloat16, device="cuda")
        res, ldo, osc = None, 0, None
    elif N == 4352:     # fc1: GELU epilogue (bf16 out for the bf16 kernel, MX out for the MX kernel)
        epi, heads, hd, hdp, tokens = pkg.lib.EPI_BIAS_GELU, 1, 8, 8, 1
        out = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
        res, ldo = None, N
        osc = torch.empty(M, N // 32, dtype=torch.uint8, device="cuda")
    else:               # out_proj / fc2: residual add, fp32 out
        epi, heads, hd, hdp, tokens = pkg.lib.EPI_RES_F32, 1, 8, 8, 1
        out = torch.empty(M, N, device="cuda")
        res, ldo, osc = torch.zeros(M, N, device="cuda"), N, None
    out2 = torch.empty(M, N, dtype=torch.bfloat16, device="cuda") if epi == pkg.lib.EPI_BIAS_GELU else None
    P = lambda t: None if t is None else t.data_ptr()  # noqa: E731

    def bf16():
        pkg.lib.check(lib.sgl_op_gemm_nt(1, A.data_ptr(), K, B.data_ptr(), K, M, N, K, epi,
                                         None if out2 is not None else out.data_ptr(), ldo, P(out2), ldo, bias.data_ptr(),
                                         P(res), N, None, 0, None, 1, tokens, heads, hd, hdp, M // tokens, s), "gemm bf16")

    def mx():
        o = out.view(torch.uint8) if epi == pkg.lib.EPI_BIAS_GELU else out
        pkg.lib.check(lib.sgl_op_gemm_nt_mx(Aq.data_ptr(), As.data_ptr(), Bq.data_ptr(), Bs.data_ptr(), M, N, Kp, epi,
                                            o.data_ptr(), ldo, P(osc), bias.data_ptr(), P(res), N, tokens, heads, hd, hdp,
                                            M // tokens, s), "gemm mx")

    times = alternate({"bf16": bf16, "mxfp8": mx}, args.blocks, args.steps, args.warmup)
    flop = 2.0 * M * N * K
    r = {m: round(flop / (median(t) * 1e-3) / 1e12, 1) for m, t in times.items()}
    r["mxfp8_over_bf16"] = round(r["mxfp8"] / r["bf16"], 4)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    pkg, oracle = entry.load_package(), entry.load_oracle()
    pkg.lib.load()
    res = {"metric": "no_grad forward img/s and NT GEMM TF/s, bf16 vs mxfp8 compute mode, one process",
           "blocks": args.blocks, "steps_per_block": args.steps, "forward": {}, "gemm_tflops_M186624": {}}
    for name, r, batch in (("so400m-patch14-384", 384, 9), ("so400m-patch14-384", 384, 64),
                           ("so400m-patch14-384", 384, 256), ("base-patch16-224", 224, 512)):
        res["forward"][f"{name}@B{batch}"] = forward_bench(pkg, name, r, batch, args)
    for N, K in ((3456, 1152), (1152, 1152), (4352, 1152), (1152, 4352)):
        res["gemm_tflops_M186624"][f"N{N}_K{K}"] = gemm_bench(pkg, 186624, N, K, args)

    cfg = pkg.get_config("so400m-patch14-384")
    sd = pkg.weights.seeded_state_dict(cfg, seed=0)
    xs = pkg.weights.seeded_pixels(2, 384, 384, seed=2)
    with torch.no_grad():
        ref = oracle.vision_forward(xs.double().cuda(), {k: v.double().cuda() for k, v in sd.items()}, cfg, False,
                                    True)["pooler_output"]
    err = {}
    for m in ("bf16", "mxfp8"):
        model = pkg.SiglipVisionModelHIP(cfg, compute_dtype=m)
        model.load_state_dict(sd)
        with torch.no_grad():
            got = model.cuda()(pixel_values=xs.cuda(), interpolate_pos_encoding=True).pooler_output.double()
        d = got - ref
        err[m] = {"max_abs": float(d.abs().max()), "rel_l2": float(d.norm() / ref.norm())}
    res["pooled_err_vs_fp32_oracle_B2"] = err
    print(json.dumps(res))


if __name__ == "__main__":
    main()
