"""Generate tests/golden/freq/ by EXECUTING THE REFERENCE'S OWN `extract_freq_vector` on real PIL crops (build container
only; the tests read only the stored numbers).

`SRM_K`, `EPS`, `_pil_to_gray256`, `fft_features`, `srm_features` and `extract_freq_vector` are lifted from the reference
app's source text with `ast` (as tests/gen_golden_views.py lifts its functions), compiled and run; nothing of the
reference is copied into this repository: only what it computed (raw 24 values, standardised vectors, gray planes) and
the seeded inputs it was given are stored.

Stated deviation: PyWavelets is not installed where this runs.  The lifted code gets a stand-in `pywt` whose
`dwt2(x, "db1")` is the 2 x 2 Haar transform with factor 1/2 (cH: detail along height, cV: along width, cD: both),
which is what db1 gives for even sizes, where no boundary extension exists; 256 and 128 are even.

    python tests/gen_golden_freq.py <reference root>

Writes sources.npz (uint8 images), expected.npz (raw, standardised, up to four cases' gray planes) and cases.json
(boxes, sha256 of every gray plane, and per feature the largest deviation of the reference's fp32 values from
tests/freq_ref.py in units of 1e-5 * |v| + 1e-8: the host test's tolerance is 1).
"""
from __future__ import annotations

import hashlib
import json
import math
import os
import sys
import types

import numpy as np
import torch
from PIL import Image, ImageOps

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import freq_ref as fr                                    # noqa: E402
from gen_golden_views import lift                        # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "freq")
LIFTED = ("SRM_K", "EPS", "_pil_to_gray256", "fft_features", "srm_features", "extract_freq_vector")
PLANES_KEPT = ("noise", "grating_r27", "multicrop_130x97")    # gray planes stored in full (first window of each)


def haar_dwt2(x, wavelet):
    assert wavelet == "db1" and x.shape[0] % 2 == 0 and x.shape[1] % 2 == 0
    p, q, r, s = x[0::2, 0::2], x[0::2, 1::2], x[1::2, 0::2], x[1::2, 1::2]
    half = x.dtype.type(0.5)
    return (p + q + r + s) * half, ((p + q - r - s) * half, (p - q + r - s) * half, (p - q - r + s) * half)


def grating(side, kx, ky, seed):
    """`kx`, `ky` cycles per image (so the peak sits at that bin of the 256 x 256 plane) plus +-8 levels of noise."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:side, 0:side]
    g = 128 + 60 * np.cos(2 * math.pi * (kx * x + ky * y) / side)
    g = g[..., None] + rng.integers(-8, 9, (side, side, 3))
    return np.clip(np.rint(g), 0, 255).astype(np.uint8)


def multicrop_boxes(w, h):
    mw, mh = w // 2, h // 2
    cx0, cy0 = (w - mw) // 2, (h - mh) // 2
    return [(cx0, cy0, cx0 + mw, cy0 + mh), (0, 0, mw, h), (w - mw, 0, w, h), (0, 0, w, mh), (0, h - mh, w, h),
            (0, 0, mw, mh), (w - mw, 0, w, mh), (0, h - mh, mw, h), (w - mw, h - mh, w, h)]


def inputs():
    """name -> (image (H, W, 3) uint8, boxes).  Geometry edges: r1 = 27.15, r2 = 81.46, sector edges on the axes and
    diagonals; the gratings sit one bin to either side."""
    rng = np.random.default_rng(20261018)
    y, x = np.mgrid[0:96, 0:128]
    smooth = 120 + 70 * np.sin(x / 23.0) * np.cos(y / 17.0) + 20 * (x / 128.0)
    smooth = np.clip(np.rint(smooth[..., None] + rng.normal(0, 6, (96, 128, 3))), 0, 255).astype(np.uint8)
    full = lambda a: [(0, 0, a.shape[1], a.shape[0])]    # noqa: E731
    cases = {"noise": rng.integers(0, 256, (120, 160, 3), dtype=np.uint8), "smooth_noise": smooth,
             "black": np.zeros((64, 64, 3), np.uint8),
             "grating_r27": grating(96, 27, 0, 1), "grating_r28": grating(96, 28, 0, 2),
             "grating_r81_in": grating(160, 65, 49, 3), "grating_r81_out": grating(160, 66, 48, 4),   # r = 81.40 / 81.61
             "grating_axis": grating(96, 20, 0, 5), "grating_diag": grating(96, 20, 20, 6)}
    out = {k: (v, full(v)) for k, v in cases.items()}
    out["multicrop_130x97"] = (rng.integers(0, 256, (97, 130, 3), dtype=np.uint8), multicrop_boxes(130, 97))
    return out


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ns = dict(torch=torch, np=np, math=math, nn=torch.nn, Image=Image, ImageOps=ImageOps, DETECT_USE_CLAHE=False,
              pywt=types.SimpleNamespace(dwt2=haar_dwt2))
    lift(os.path.join(sys.argv[1], "appv3.py"), LIFTED, ns)
    os.makedirs(OUT, exist_ok=True)
    sources, expected, doc = {}, {}, {"source": "appv3.py extract_freq_vector on PIL crops; pywt.dwt2 replaced by 2x2 Haar",
                                      "features": fr.NAMES, "cases": {}}
    worst = np.zeros(24)
    for name, (img, boxes) in inputs().items():
        pil = Image.fromarray(img)
        raw, std, shas = [], [], []
        for n, box in enumerate(boxes):
            crop = pil.crop(box)
            raw.append(np.array(ns["fft_features"](crop)[0] + ns["srm_features"](crop), dtype=np.float64))
            std.append(ns["extract_freq_vector"](crop).numpy())
            plane = np.asarray(crop.convert("L").resize((256, 256), Image.BICUBIC))
            assert np.array_equal(np.rint(ns["_pil_to_gray256"](crop).numpy() * 255).astype(np.uint8), plane)
            shas.append(hashlib.sha256(plane.tobytes()).hexdigest())
            if n == 0 and name in PLANES_KEPT:
                expected[f"{name}.gray"] = plane
            mine = fr.raw_features(fr.gray256(img, box))
            worst = np.maximum(worst, np.abs(raw[-1] - mine) / (1e-5 * np.abs(mine) + 1e-8))
        sources[name] = img
        expected[f"{name}.raw"] = np.stack(raw)
        expected[f"{name}.std"] = np.stack(std).astype(np.float32)
        doc["cases"][name] = {"boxes": [list(b) for b in boxes], "gray_sha256": shas}
    doc["fp32_reference_vs_freq_ref_in_tolerances"] = {k: round(float(v), 4) for k, v in zip(fr.NAMES, worst)}
    np.savez_compressed(os.path.join(OUT, "sources.npz"), **sources)
    np.savez_compressed(os.path.join(OUT, "expected.npz"), **expected)
    with open(os.path.join(OUT, "cases.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc["fp32_reference_vs_freq_ref_in_tolerances"], indent=1))


if __name__ == "__main__":
    main()
