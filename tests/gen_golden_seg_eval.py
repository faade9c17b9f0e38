"""Generate tests/golden/seg_eval/ by EXECUTING THE REFERENCE'S OWN `dice_iou_from_logits` and `sweep_mask_thresholds`
(build container only; the tests read only the stored data).

The two functions are lifted from the reference's source text with `ast` (as tests/gen_golden_views.py does), compiled and
run on `F.interpolate(lr, (S, S), 'bilinear', align_corners=False)` of seeded low-resolution logits; nothing of the reference
is copied into this repository: only numbers are stored.  Per case `<name>.npz` holds

    lr              (B, g, g) fp32 low-res logits            masks_packed    np.packbits of the (B, S, S) {0,1} masks
    cuts            the K sorted fp32 logit cuts             sweep_index     cut of each of the 17 sweep thresholds
    ref_f1/dice/iou per sweep threshold, what the reference's sweep computed (F1 by sklearn, mean Dice / IoU)
    ref_dice_at / ref_iou_at   mean per-image Dice / IoU of dice_iou_from_logits at EXTRA_THR (0.5, 0.37)
    f1_dev/dice_dev/iou_dev    per cut, the most the borderline pixels could move each number
    hist            (B, 2, K+1) float64-logit pixel counts   borderline      (B, K) pixels within 2^-16 max(1,|z|) of a cut
    auc_bins        (2, 4096) float64-logit AUC histogram    auc_sklearn     roc_auc_score over all masked pixels, float64
    auc_near_edge   pixels within the margin of an AUC bin edge

and `cases.json` the shapes, `has_mask`, the thresholds and the reference's `best` dict.  The generator ASSERTS what the
tests rely on (max |z| <= 16; borderline share <= 1e-4; the fp32 reference and the float64 counts agree to 1e-6 at every
threshold; each best threshold beats every other by more than the borderline pixels could move either) and tries the next
seed when a condition fails.

    python tests/gen_golden_seg_eval.py <reference root>
"""
from __future__ import annotations

import json
import os
import sys
from typing import List

import numpy as np
import torch
import torch.nn.functional as F
from sklearn.metrics import f1_score, roc_auc_score

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seg_eval_ref as R                     # noqa: E402
from gen_golden_views import lift            # noqa: E402

THR = dict(thr_min=0.1, thr_max=0.9, thr_steps=17)        # the reference's defaults (:204-207)
EXTRA_THR = (0.5, 0.37)                                     # --mask_thr's default, and one that is no sweep threshold
# (B, g, S), what each image is: blobs / bg (all background) / fg (all foreground) / nomask (blobs, has_mask False)
CASES = [("odd17", 2, 3, 17, ("blobs", "bg")), ("mid96", 3, 7, 96, ("blobs", "nomask", "blobs")),
         ("base224", 2, 14, 224, ("blobs", "fg")), ("so400m384", 2, 27, 384, ("blobs", "blobs")),
         ("single5", 1, 1, 5, ("blobs",))]


def make_case(B, g, S, kinds, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:S, 0:S]
    masks = np.zeros((B, S, S), dtype=np.uint8)
    for b, kind in enumerate(kinds):
        if kind == "fg":
            masks[b] = 1
        elif kind != "bg":
            for _ in range(int(rng.integers(1, 4))):
                cy, cx = rng.uniform(0.15, 0.85, 2) * S
                ry, rx = rng.uniform(0.12, 0.3, 2) * S + 0.6
                masks[b] |= (((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0).astype(np.uint8)
    coarse = F.adaptive_avg_pool2d(torch.from_numpy(masks).float()[:, None], (g, g))[:, 0].numpy()
    lr = (coarse * 4.0 - 1.4 + rng.normal(0.0, 1.0, (B, g, g))).astype(np.float32)        # correlated with the mask
    return lr, masks, np.array([k != "nomask" for k in kinds])


def run_reference(ns, lr, masks, has_mask, S):
    """The reference's sweep on the masked images, with its per-threshold numbers recorded on the way."""
    up = F.interpolate(torch.from_numpy(lr)[:, None], size=(S, S), mode="bilinear", align_corners=False)
    hm = torch.from_numpy(has_mask)
    seg, m = up[hm], torch.from_numpy(masks).float()[:, None][hm]
    rec = {"f1": [], "dice": [], "iou": []}
    inner = ns["dice_iou_from_logits"]

    def recording_dice_iou(*a, **k):
        d, i, p = inner(*a, **k)
        rec["dice"].append(float(np.mean(d)))
        rec["iou"].append(float(np.mean(i)))
        rec["f1"].append(0.0)                     # overwritten when the reference calls f1_score for this threshold
        return d, i, p

    def recording_f1(*a, **k):
        v = f1_score(*a, **k)
        rec["f1"][-1] = float(v)
        return v
    run = dict(ns, dice_iou_from_logits=recording_dice_iou, f1_score=recording_f1)
    sweep = type(ns["sweep_mask_thresholds"])(ns["sweep_mask_thresholds"].__code__, run, "sweep_mask_thresholds",
                                              ns["sweep_mask_thresholds"].__defaults__)
    half = max(1, seg.shape[0] // 2)              # two "batches", as the validation loop collects them
    best = sweep([seg[:half], seg[half:]] if seg.shape[0] > 1 else [seg], [m[:half], m[half:]] if seg.shape[0] > 1 else [m],
                 **THR)
    at = {}
    for thr in EXTRA_THR:
        d, i, _ = inner(seg, m, thr=thr)
        at[thr] = (float(np.mean(d)), float(np.mean(i)))
    return {k: (float(v)) for k, v in best.items()}, rec, at


def stable(curve, dev, order, eps=0.0):
    """The first maximum in scan order beats every other threshold by more than both could move, or ties it exactly, later
    in the scan, with nothing borderline at either."""
    vals = [curve[j] for j in order]
    k = int(np.argmax(vals))                       # first maximum
    if vals[k] <= 0:
        return False
    for pos, j in enumerate(order):
        if pos == k:
            continue
        if curve[j] + dev[j] < vals[k] - dev[order[k]]:
            continue
        if pos > k and curve[j] == vals[k] and dev[j] == 0 and dev[order[k]] == 0:
            continue
        return False
    return True


def build(ns, name, B, g, S, kinds):
    thresholds = np.linspace(THR["thr_min"], THR["thr_max"], THR["thr_steps"])
    cuts, index = R.cuts_for(np.concatenate([thresholds, EXTRA_THR]))
    sweep_index, extra_index = index[:len(thresholds)], index[len(thresholds):]
    for seed in range(100, 140):
        lr, masks, has_mask = make_case(B, g, S, kinds, seed)
        z = R.upsample64(lr, S)
        if np.abs(z).max() > 16:
            continue
        hist = R.hist64(z, masks, cuts, has_mask)
        border = R.borderline(z, cuts, has_mask)
        if border.sum() > 1e-4 * has_mask.sum() * S * S * len(cuts):
            continue
        cur = R.curves_from_hist(hist, has_mask, border)
        best, rec, at = run_reference(ns, lr, masks, has_mask, S)
        agree = all(np.abs(np.asarray(rec[k]) - cur[k][sweep_index]).max() <= 1e-6 for k in ("f1", "dice", "iou"))
        agree = agree and all(abs(at[t][0] - cur["dice"][j]) <= 1e-6 and abs(at[t][1] - cur["iou"][j]) <= 1e-6
                              for t, j in zip(EXTRA_THR, extra_index))
        if not agree or not all(stable(cur[k], cur[k + "_dev"], list(sweep_index)) for k in ("f1", "dice", "iou")):
            continue
        mine = R.best_from_curves(thresholds, *(cur[k][sweep_index] for k in ("f1", "dice", "iou")))
        assert all(abs(mine[k] - best[k]) <= 1e-6 for k in best), (mine, best)
        bins, near = R.auc_bins(z, masks, has_mask)
        auc = float(roc_auc_score(masks[has_mask].reshape(-1), z[has_mask].reshape(-1)))
        a, hw = R.auc_from_bins(bins)
        assert abs(a - auc) <= hw + 1e-12, (a, auc, hw)
        arrays = dict(lr=lr, masks_packed=R.pack_masks(masks), cuts=cuts, sweep_index=sweep_index, extra_index=extra_index,
                      ref_f1=np.asarray(rec["f1"]), ref_dice=np.asarray(rec["dice"]), ref_iou=np.asarray(rec["iou"]),
                      ref_dice_at=np.asarray([at[t][0] for t in EXTRA_THR]),
                      ref_iou_at=np.asarray([at[t][1] for t in EXTRA_THR]), f1_dev=cur["f1_dev"], dice_dev=cur["dice_dev"],
                      iou_dev=cur["iou_dev"], hist=hist, borderline=border, auc_bins=bins, auc_sklearn=np.float64(auc),
                      auc_near_edge=np.int64(near))
        meta = {"name": name, "B": B, "g": g, "S": S, "kinds": list(kinds), "has_mask": [bool(v) for v in has_mask],
                "seed": seed, "best": best, "borderline_total": int(border.sum()), "max_abs_z": float(np.abs(z).max())}
        return meta, arrays
    raise SystemExit(f"{name}: no seed met the conditions")


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ns = dict(torch=torch, np=np, F=F, List=List, f1_score=f1_score)
    lift(os.path.join(sys.argv[1], "Siglip2sidafrozen.py"), ("dice_iou_from_logits", "sweep_mask_thresholds"), ns)
    os.makedirs(R.GOLDEN_DIR, exist_ok=True)
    metas = []
    for name, B, g, S, kinds in CASES:
        meta, arrays = build(ns, name, B, g, S, kinds)
        np.savez_compressed(os.path.join(R.GOLDEN_DIR, name + ".npz"), **arrays)
        metas.append(meta)
        print(f"{name}: seed {meta['seed']} borderline {meta['borderline_total']} best {meta['best']}")
    doc = {"source": "Siglip2sidafrozen.py dice_iou_from_logits / sweep_mask_thresholds run on F.interpolate of seeded "
                     "low-res logits; sklearn f1_score / roc_auc_score",
           "thresholds": THR, "extra_thresholds": list(EXTRA_THR), "cases": metas}
    with open(os.path.join(R.GOLDEN_DIR, "cases.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
