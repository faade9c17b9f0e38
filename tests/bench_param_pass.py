"""Developer micro-benchmark of the parameter-side passes through the C ABI at so400m sizes (not part of the test-suite).
   python tests/bench_param_pass.py [reps]   -> one JSON line of event-timed medians, milliseconds:
     prepare_weights_ms   sgl_prepare_weights over all 27 blocks + globals (bf16 shadows)
     grad_norm_ms         sgl_op_grad_norm over every parameter (two launches)
     ema_ms               sgl_op_ema over every parameter
     adamw_ms             sgl_op_adamw over every parameter
     split3_rows_ms / split3_stack_ms    sgl_op_split3 of a 93312 x 1152 fp32 operand (B = 128 tokens x hidden)"""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import __graft_entry__ as g

pkg = g.load_package(); L = pkg.lib; lib = L.load()
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
dev = torch.device("cuda:0")
st = torch.cuda.current_stream()


def median_ms(fn, warmup=3):
    for _ in range(warmup): fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st); fn(); e1.record(st); e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return round(sorted(ts)[len(ts) // 2], 4)


cfg = pkg.get_config("so400m-patch14-384")
model = pkg.SiglipVisionModelHIP(cfg, compute_dtype="bf16").to(dev)
with torch.no_grad():
    model(pixel_values=torch.zeros(1, 3, cfg.image_size, cfg.image_size, device=dev))     # allocates the shadow arena
ctx, wts, arena = model._shadows.binding()
out = {}
out["prepare_weights_ms"] = median_ms(lambda: L.check(
    lib.sgl_prepare_weights(ctx, C.byref(wts), arena.data_ptr(), arena.numel(), st.cuda_stream), "sgl_prepare_weights"))

params = list(model.parameters())
table = (L.SglAdamwTensor * len(params))()
keep = []
for e, p in zip(table, params):
    gr, m, v = torch.randn_like(p) * 1e-3, torch.zeros_like(p), torch.zeros_like(p)
    keep += [gr, m, v]
    e.p, e.g, e.m, e.v, e.n, e.lr, e.weight_decay = p.data_ptr(), gr.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), 1e-5, 0.01
numel = (C.c_uint64 * len(params))(*[p.numel() for p in params])
nb = lib.sgl_adamw_plan(numel, len(params), None, 0)
bm = (C.c_int32 * (2 * nb))()
lib.sgl_adamw_plan(numel, len(params), bm, nb)
dtab = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(dev)
bmap = torch.frombuffer(bytearray(bytes(bm)), dtype=torch.int32).to(dev)
partials, norm = torch.empty(nb, device=dev), torch.zeros(2, device=dev)
out["grad_norm_ms"] = median_ms(lambda: L.call("sgl_op_grad_norm", dev, dtab.data_ptr(), bmap.data_ptr(), nb, 1.0,
                                               partials.data_ptr(), norm.data_ptr()))
out["ema_ms"] = median_ms(lambda: L.call("sgl_op_ema", dev, dtab.data_ptr(), bmap.data_ptr(), nb, 0.9999))
out["adamw_ms"] = median_ms(lambda: L.call("sgl_op_adamw", dev, dtab.data_ptr(), bmap.data_ptr(), nb, 0.9, 0.999, 1e-8, 1,
                                           norm.data_ptr()))

R, Cc = 128 * 729, 1152
src = torch.randn(R, Cc, device=dev)
dst = torch.empty(3 * R * Cc, device=dev, dtype=torch.bfloat16)
for stacked, name in ((0, "split3_rows_ms"), (1, "split3_stack_ms")):
    out[name] = median_ms(lambda: L.call("sgl_op_split3", dev, src.data_ptr(), R, Cc, Cc, dst.data_ptr(), Cc, 0, stacked))
out.update(parameters=sum(p.numel() for p in params), blocks=nb, reps=reps, device=torch.cuda.get_device_name(0))
print(json.dumps(out))
