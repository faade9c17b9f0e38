"""Generate tests/golden/app_views.json by EXECUTING THE REFERENCE'S OWN `make_multicrops` and `compute_patch_grid`
(build container only; the tests read only the JSON).

The two functions are lifted from the reference app's source text with `ast` (the way oracle/gen_golden_heads.py lifts
classes), compiled and run on a stub image that records every `.crop` box; nothing of the reference is copied into this
repository: only the numbers it produced (boxes, weights) are stored.

    python tests/gen_golden_views.py <reference root>
"""
from __future__ import annotations

import ast
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "app_views.json")
SIZES = [(64, 64), (97, 64), (65, 130), (640, 427), (1031, 777), (2048, 1365), (3, 9)]       # (w, h), PIL's order
CONSTANTS = ("IMG_SIZE", "MIN_SIDE", "PATCH_GRID_ROWS", "PATCH_GRID_COLS")


def lift(path, names, ns):
    """exec the top-level FunctionDef / Assign nodes called `names` (in file order) from `path` into `ns`."""
    tree = ast.parse(open(path, encoding="utf-8").read())
    want, seen = set(names), set()
    for node in tree.body:
        key = None
        if isinstance(node, ast.FunctionDef) and node.name in want:
            key = node.name
        elif isinstance(node, ast.Assign) and len(node.targets) == 1 and isinstance(node.targets[0], ast.Name) \
                and node.targets[0].id in want:
            key = node.targets[0].id
        if key is None or key in seen:
            continue
        seen.add(key)
        exec(compile(ast.Module(body=[node], type_ignores=[]), f"<ref:{os.path.basename(path)}:{node.lineno}>", "exec"), ns)
    assert want == seen, f"{path}: not found {want - seen}"


class StubImage:
    """Stands in for a PIL image: a size, and a log of the boxes `.crop` was asked for."""

    def __init__(self, size, log):
        self.size, self.log = tuple(size), log
        self.width, self.height = self.size

    def crop(self, box):
        box = [int(v) for v in box]
        self.log.append(box)
        return StubImage((box[2] - box[0], box[3] - box[1]), [])

    def resize(self, size, *args, **kwargs):
        self.log.append({"resize": [int(v) for v in size]})
        return StubImage(size, [])


class StubFilters:
    BICUBIC = BILINEAR = NEAREST = 0


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ns = dict(torch=torch, np=np, Image=StubFilters, detect_core=lambda *a, **k: {"p_fake_raw": 1.0})
    app = os.path.join(sys.argv[1], "appv3.py")
    lift(app, CONSTANTS, ns)
    lift(app, ("make_multicrops", "compute_patch_grid"), ns)
    cases = []
    for w, h in SIZES:
        log = []
        crops, weights = ns["make_multicrops"](StubImage((w, h), log))
        fallback = [e for e in log if isinstance(e, dict)]
        case = {"w": w, "h": h, "multicrop_boxes": [e for e in log if not isinstance(e, dict)],
                "multicrop_fallback_resize": fallback[0]["resize"] if fallback else None,
                "weights": [float(np.float32(v)) for v in weights.tolist()], "num_crops": len(crops)}
        log = []
        grid, scores = ns["compute_patch_grid"](StubImage((w, h), log), None, None)
        if grid is None:
            case["grid"] = None
        else:
            live = (np.asarray(grid) > 0).reshape(-1).tolist()
            boxes = iter(log)
            case["grid"] = {"rows": int(grid.shape[0]), "cols": int(grid.shape[1]),
                            "cells": [next(boxes) if on else None for on in live]}
            assert next(boxes, None) is None and len(scores) == len(live)
        cases.append(case)
    doc = {"source": "appv3.py make_multicrops / compute_patch_grid run on a box-recording stub image",
           "constants": {k: ns[k] for k in CONSTANTS}, "cases": cases}
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"wrote {OUT}: {len(cases)} sizes")


if __name__ == "__main__":
    main()
