"""Developer micro-benchmark of the optimizer step tail under torch.amp.GradScaler on the so400m parameter set, with the
encoder's weight shadows attached (not part of the test-suite).
   python tests/bench_amp_step.py [reps]   -> one JSON line, also written to profiles/amp_step_bench.json
Per variant the median over `reps` (default 10) of the event-timed step tail in milliseconds (`*_ms`: from the first launch
to the last kernel's end, a host stall between launches included) and of its wall time with a final synchronisation
(`*_wall_ms`).  The gradients are loss-scaled by 65536 and restored from a master copy before every repetition, outside
the timed region (unscale_ and clip_grad_norm_ write them).
     a_five_lines_parent   scaler.unscale_(opt); clip_grad_norm_(params, 1.0); scaler.step(opt); scaler.update() with an
                           optimizer that does not announce `_step_supports_amp_scaling`: the route of the tree before the
                           protocol (GradScaler calls found_inf.item(), then the plain step)
     b_five_lines          the same five lines with FusedAdamW as it is now (the skip is decided on the device)
     c_stock_short         FusedAdamW(max_grad_norm=1.0); torch.amp.GradScaler: scaler.step(opt); scaler.update()
     d_amd_short           the same with siglip_amd.GradScaler (no separate inf check pass)
     floor_unscaled        FusedAdamW(max_grad_norm=1.0).step() on unscaled gradients, no scaler"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import __graft_entry__ as g

pkg = g.load_package()
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
dev = torch.device("cuda:0")
st = torch.cuda.current_stream()
SCALE, CLIP = 65536.0, 1.0

cfg = pkg.get_config("so400m-patch14-384")
model = pkg.SiglipVisionModelHIP(cfg, compute_dtype="bf16").to(dev)
with torch.no_grad():
    model(pixel_values=torch.zeros(1, 3, cfg.image_size, cfg.image_size, device=dev))     # allocates the shadow arena
params = list(model.parameters())
gen = torch.Generator(device=dev).manual_seed(0)
master = [torch.randn(p.shape, device=dev, generator=gen) * 1e-3 for p in params]
for p in params:
    p.grad = torch.empty_like(p)


def restore(scale):
    torch._foreach_copy_([p.grad for p in params], master)
    if scale != 1.0:
        torch._foreach_mul_([p.grad for p in params], scale)


class ParentRoute(pkg.FusedAdamW):
    _step_supports_amp_scaling = False


def measure(make_opt, make_scaler, tail, scale):
    opt = make_opt().attach_encoder(model)
    scaler = make_scaler() if make_scaler else None
    if scaler is not None:
        scaler.scale(torch.ones((), device=dev))        # the scale tensor is created by the first scale() call
    ev, wall = [], []
    for i in range(3 + reps):
        restore(scale)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record(st)
        tail(opt, scaler)
        e1.record(st)
        e1.synchronize()
        t1 = time.perf_counter()
        if i >= 3:
            ev.append(e0.elapsed_time(e1))
            wall.append((t1 - t0) * 1e3)
    if scaler is not None:
        assert scaler.get_scale() == SCALE, "a step was skipped"
    del opt
    torch.cuda.empty_cache()
    return round(sorted(ev)[len(ev) // 2], 4), round(sorted(wall)[len(wall) // 2], 4)


def five_lines(opt, scaler):
    scaler.unscale_(opt)
    torch.nn.utils.clip_grad_norm_(params, CLIP)
    scaler.step(opt)
    scaler.update()


def short(opt, scaler):
    scaler.step(opt)
    scaler.update()


def plain(lr_only=False, cls=pkg.FusedAdamW):
    return lambda: cls(params, lr=1e-5, weight_decay=0.01, max_grad_norm=None if lr_only else CLIP)


stock = lambda: torch.amp.GradScaler("cuda", init_scale=SCALE)
out = {}
for name, args in (
        ("a_five_lines_parent", (plain(True, ParentRoute), stock, five_lines, SCALE)),
        ("b_five_lines", (plain(True), stock, five_lines, SCALE)),
        ("c_stock_short", (plain(), stock, short, SCALE)),
        ("d_amd_short", (plain(), lambda: pkg.GradScaler("cuda", init_scale=SCALE), short, SCALE)),
        ("floor_unscaled", (plain(), None, lambda opt, _: opt.step(), 1.0))):
    out[name + "_ms"], out[name + "_wall_ms"] = measure(*args)
out.update(parameters=sum(p.numel() for p in params), reps=reps, loss_scale=SCALE,
           device=torch.cuda.get_device_name(0))
line = json.dumps(out)
print(line)
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "amp_step_bench.json"), "w") as f:
    f.write(line + "\n")
