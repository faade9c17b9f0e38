"""What the app's frequency / SRM feature vectors cost: the 25 windows `detect_core` takes them from (9 crops and 16 grid
cells of `preprocess.detect_views`) of one 1024 x 1024 uint8 image.  One process, warmed up, medians.

Legs:  a  preprocess.views_freq_features: one sgl_op_freq_features pass (seven launches), event-timed on the stream;
          and the bare C call on preallocated buffers (no allocation, no table packing)
       b  the host route the app runs today, restated from tests/freq_ref.py in the app's own precision: per window PIL
          crop -> convert("L") -> resize(256, BICUBIC), torch fp32 fft2 and mask reductions with their `.item()` round
          trips, numpy Haar, three conv2d, standardise; a host clock, with the number of CPUs the process may use.
          The radius / bucket / sector masks are built once outside the clock (the app rebuilds them per window), so
          this leg flatters the host.

No ratio is fixed in advance; whether (a) beats (b) is recorded as it comes out.  Prints ONE JSON line; --out writes it.

    python tests/bench_freq.py [--blocks 4] [--steps 10] [--warmup 3] [--out profiles/freq_bench.json]
"""
import argparse
import json
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__ as entry  # noqa: E402
import freq_ref as fr  # noqa: E402
from bench_input_grad import median, timed  # noqa: E402


def stats(t, nd=4):
    return {"ms_median": round(median(t), nd), "ms_min": round(min(t), nd), "ms_max": round(max(t), nd), "runs": len(t)}


def host_vector(Image, np, crop, masks, srm):
    """One window the way the app computes it: fp32 torch on the host, a Python float per reduction."""
    band, bucket, sector = masks
    x = torch.from_numpy(np.asarray(crop.convert("L").resize((256, 256), Image.BICUBIC), dtype=np.float32) / 255.0)
    F = torch.fft.fftshift(torch.fft.fft2(x))
    mag, phase = torch.abs(F), torch.angle(F)
    Et = float(mag.sum().item()) + 1e-6
    El, Em, Eh = (float(mag[m].sum().item()) for m in band)
    flat = mag.flatten()
    mu = [float(torch.log(flat[m] + 1e-6).mean().item()) if m.any() else 0.0 for m in bucket]
    slope = float(np.polyfit(np.arange(len(mu)), np.asarray(mu), 1)[0])
    hist = torch.histc(phase.flatten(), bins=50, min=-math.pi, max=math.pi)
    prob = hist / (hist.sum() + 1e-6)
    entropy = float(-(prob * torch.log(prob + 1e-6)).sum().item())
    anis = float(np.var([float(mag[m].mean().item()) for m in sector]))
    a = x.numpy()
    wave = []
    for _ in range(2):
        p, q, r, s = a[0::2, 0::2], a[0::2, 1::2], a[1::2, 0::2], a[1::2, 1::2]
        cs = [(p + q + r + s) * 0.5, (p + q - r - s) * 0.5, (p - q + r - s) * 0.5, (p - q - r + s) * 0.5]
        wave += [float(np.mean(np.abs(c) ** 2)) for c in cs]
        a = cs[0]
    feats = [El / Et, Em / Et, Eh / Et, (Eh + 1e-6) / (El + 1e-6), slope, anis, entropy] + wave
    for k in srm:
        y = torch.nn.functional.conv2d(x[None, None], k, padding=k.shape[-1] // 2).flatten().numpy()
        m, v = float(y.mean()), float(y.var())
        feats += [m, v, float(((y - m) ** 4).mean() / ((v + 1e-6) ** 2))]
    v = torch.tensor(feats, dtype=torch.float32)
    return v * 0.0 if v.std() < 1e-6 else (v - v.mean()) / (v.std() + 1e-6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--side", type=int, default=1024)
    ap.add_argument("--no-host", action="store_true", help="GPU legs only (for a kernel-trace run)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_freq.py measures on the GPU only"
    pkg = entry.load_package()
    lib = pkg.lib.load()
    pp = pkg.preprocess
    dev = torch.device("cuda")
    st = torch.cuda.current_stream()
    s = pkg.lib.current_stream_handle(dev)
    h = w = args.side
    img = torch.randint(0, 256, (1, h, w, 3), generator=torch.Generator().manual_seed(h + w), dtype=torch.uint8)
    src = img.cuda()
    d = pp.detect_views(h, w)
    views = [d.views[n] for n in d.freq]
    V = len(views)
    assert V == 25
    tab = pp.view_table(views, 1, h, w)
    geom = pp.freq_geometry_on(dev)
    out = torch.empty(V, 24, device=dev)
    nbytes = lib.sgl_op_freq_features_scratch_bytes(V, h, w)
    scratch = torch.empty(nbytes, device=dev, dtype=torch.uint8)

    def c_call():
        assert lib.sgl_op_freq_features(src.data_ptr(), 1, h, w, tab, V, geom.data_ptr(), out.data_ptr(), 1, None,
                                        scratch.data_ptr(), nbytes, s) == 0

    def python_entry():
        pp.views_freq_features(src, views)

    legs = {"a_c_call_preallocated": c_call, "a_views_freq_features": python_entry}
    names = list(legs)
    for n in names:
        for _ in range(args.warmup):
            legs[n]()
    torch.cuda.synchronize()
    times = {n: [] for n in names}
    for blk in range(args.blocks):
        for n in (names if blk % 2 == 0 else names[::-1]):
            times[n] += timed(legs[n], args.steps, st)
    res = {"metric": "the app's 24-D frequency / SRM vectors of the 25 windows detect_core takes them from, one uint8 image; "
                     "GPU legs event-timed medians alternating in blocks, host leg a host clock",
           "views": V, "source_wh": [w, h], "blocks": args.blocks, "steps_per_block": args.steps, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(0), "scratch_bytes": nbytes}
    for n in names:
        res[n] = stats(times[n])
    got = pp.views_freq_features(src, views).cpu()

    try:
        from PIL import Image
        import numpy as np
    except ImportError:
        Image = np = None
    if args.no_host:
        res["b_host_route"] = "not measured: --no-host"
    elif Image is not None:
        tables = fr.geometry()
        masks = ([tables[0] == b for b in range(3)], [(tables[1] == b).flatten() for b in range(39)],
                 [tables[2] == b for b in range(8)])
        srm = [torch.tensor(k, dtype=torch.float32) for k in fr.SRM]
        srm = [(k / (k.abs().sum() + 1e-6)).view(1, 1, *k.shape) for k in srm]
        pil = Image.fromarray(img[0].numpy())
        host, vecs = [], None
        for i in range(2 + 20):
            t0 = time.perf_counter()
            vecs = torch.stack([host_vector(Image, np, pil.crop(v.box), masks, srm) for v in views]).to(dev)
            torch.cuda.synchronize()
            if i >= 2:
                host.append((time.perf_counter() - t0) * 1e3)
        res["b_host_route"] = dict(stats(host, 2), cpus_in_affinity_mask=len(os.sched_getaffinity(0)),
                                   torch_threads=torch.get_num_threads(),
                                   note="masks prebuilt outside the clock (the app rebuilds them per window)")
        res["max_abs_difference_gpu_vs_host_route"] = round(float((vecs.cpu() - got).abs().max()), 7)
        a, b = res["a_views_freq_features"]["ms_median"], res["b_host_route"]["ms_median"]
        res["b_over_a"] = round(b / a, 1)
        res["gpu_not_slower_than_host"] = bool(a <= b)
    else:
        res["b_host_route"] = "not measured: PIL is not importable"
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
