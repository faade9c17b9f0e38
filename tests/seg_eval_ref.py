"""float64 reference of the mask localisation metrics (csrc/decoder_tail.hip: seg_eval, heads.MaskMetrics), independent of
the package: numpy only.  A plain module: no tests, no fixtures.

* ``upsample64``       bilinear, align_corners=False, in float64 (PyTorch's upsample_bilinear2d index rule)
* ``cuts_for``         logit(float32(thr)) formed in float64 and rounded to fp32: ``sigmoid(z) > thr`` as ``z > cut``
* ``hist64``           per (image, class, bin): pixels whose logit has exactly k cuts strictly below it
* ``borderline``       per (image, cut): pixels with |z - cut| < 2^-16 max(1, |z|), the ones an fp32 evaluation of z (a few
                       ulp(16) = 1.9e-6 off for |z| <= 16, so under 2^-16) may put on the other side of the cut
* ``curves_from_hist`` per-cut global F1 and mean per-image Dice / IoU from the counts, with the most each can move when up
                       to m[b, j] pixels of image b change sides at cut j
* ``best_from_curves`` the reference's selection rule (scan order, strict >, from 0 with threshold 0.5)
* ``auc_bins`` / ``auc_from_bins``  the 4096-bin logit histogram on [-16, 16) and the AUC with in-bin ties counted one half
* ``pack_masks`` / ``unpack_masks``  np.packbits storage of {0,1} masks
"""
from __future__ import annotations

import json
import os

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "seg_eval")
NB = 4096
MARGIN = 2.0 ** -16


def _src(n_out, n_in):
    s = np.maximum((n_in / n_out) * (np.arange(n_out, dtype=np.float64) + 0.5) - 0.5, 0.0)
    i0 = np.minimum(np.floor(s).astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, s - i0


def upsample64(lr, S):
    """(B, g, g) -> (B, S, S) float64."""
    lr = np.asarray(lr, dtype=np.float64)
    g = lr.shape[-1]
    i0, i1, w = _src(S, g)
    rows = lr[:, i0, :] * (1.0 - w)[None, :, None] + lr[:, i1, :] * w[None, :, None]
    return rows[:, :, i0] * (1.0 - w)[None, None, :] + rows[:, :, i1] * w[None, None, :]


def cuts_for(thresholds):
    """(sorted unique fp32 cuts, index of each threshold's cut)."""
    t32 = np.asarray(thresholds, dtype=np.float64).astype(np.float32).astype(np.float64)
    cuts, index = np.unique(np.log(t32 / (1.0 - t32)).astype(np.float32), return_inverse=True)
    return cuts, index.astype(np.int64)


def hist64(z, masks, cuts, has_mask=None):
    """(B, 2, K+1) int64; rows of images with has_mask False are zero."""
    B = z.shape[0]
    K = len(cuts)
    out = np.zeros((B, 2, K + 1), dtype=np.int64)
    c64 = np.asarray(cuts, dtype=np.float64)
    for b in range(B):
        if has_mask is not None and not has_mask[b]:
            continue
        k = np.searchsorted(c64, z[b].reshape(-1), side="left")       # number of cuts strictly below z
        cls = (np.asarray(masks[b]).reshape(-1) > 0.5).astype(np.int64)
        np.add.at(out[b], (cls, k), 1)
    return out


def borderline(z, cuts, has_mask=None):
    """(B, K) int64."""
    B = z.shape[0]
    out = np.zeros((B, len(cuts)), dtype=np.int64)
    for b in range(B):
        if has_mask is not None and not has_mask[b]:
            continue
        zb = z[b].reshape(-1)
        tol = MARGIN * np.maximum(1.0, np.abs(zb))
        for j, c in enumerate(np.asarray(cuts, dtype=np.float64)):
            out[b, j] = int((np.abs(zb - c) < tol).sum())
    return out


def _ratio(tp, fp, fg, eps):
    """Dice 2tp/(tp+fp+fg+eps) and IoU tp/(fp+fg+eps): both rise with tp and fall with fp."""
    return 2.0 * tp / (tp + fp + fg + eps), tp / (fp + fg + eps)


def curves_from_hist(hist, has_mask=None, m=None, eps=1e-6):
    """Per cut j: global F1 (0 when the masks are all one value), mean over masked images of Dice and IoU, and for each the
    largest change possible when up to m[b, j] pixels of image b are predicted the other way."""
    h = np.asarray(hist, dtype=np.float64)
    B, _, K1 = h.shape
    keep = np.ones(B, bool) if has_mask is None else np.asarray(has_mask, bool)
    h = h[keep]
    m = np.zeros((len(h), K1 - 1)) if m is None else np.asarray(m, dtype=np.float64)[keep]
    above = np.cumsum(h[:, :, ::-1], axis=-1)[:, :, ::-1]
    tp, fp = above[:, 1, 1:], above[:, 0, 1:]
    fg, bg = above[:, 1, 0][:, None], above[:, 0, 0][:, None]
    n = max(len(h), 1)

    def per_image(tp_, fp_):
        d, i = _ratio(tp_, fp_, fg, eps)
        return d.sum(0) / n, i.sum(0) / n
    dice, iou = per_image(tp, fp)
    hi = per_image(np.minimum(tp + m, fg), np.maximum(fp - m, 0.0))
    lo = per_image(np.maximum(tp - m, 0.0), np.minimum(fp + m, bg))
    TP, FP, FG, BG, M = tp.sum(0), fp.sum(0), fg.sum(), bg.sum(), m.sum(0)

    def f1_of(TP_, FP_):
        den = TP_ + FP_ + FG                                           # 2TP + FP + FN
        return np.where(den > 0, 2.0 * TP_ / np.maximum(den, 1.0), 0.0) if FG > 0 and BG > 0 else np.zeros_like(TP_)
    f1 = f1_of(TP, FP)
    f1_hi, f1_lo = f1_of(np.minimum(TP + M, FG), np.maximum(FP - M, 0.0)), f1_of(np.maximum(TP - M, 0.0),
                                                                                 np.minimum(FP + M, BG))
    dev = lambda v, a, b: np.maximum(np.abs(a - v), np.abs(b - v))
    return {"f1": f1, "dice": dice, "iou": iou, "f1_dev": dev(f1, f1_hi, f1_lo), "dice_dev": dev(dice, hi[0], lo[0]),
            "iou_dev": dev(iou, hi[1], lo[1])}


def best_from_curves(thresholds, f1, dice, iou):
    best = {"f1": 0, "dice": 0, "iou": 0, "thr_f1": 0.5, "thr_dice": 0.5, "thr_iou": 0.5}
    for t, vals in zip(thresholds, zip(f1, dice, iou)):
        for name, v in zip(("f1", "dice", "iou"), vals):
            if v > best[name]:
                best[name], best["thr_" + name] = float(v), float(t)
    return best


def auc_bins(z, masks, has_mask=None):
    """((2, NB) int64 [background, foreground], pixels within the margin of a bin edge)."""
    out = np.zeros((2, NB), dtype=np.int64)
    near = 0
    for b in range(z.shape[0]):
        if has_mask is not None and not has_mask[b]:
            continue
        zb = z[b].reshape(-1)
        f = (zb + 16.0) * (NB / 32.0)
        bins = np.clip(np.floor(f), 0, NB - 1).astype(np.int64)
        cls = (np.asarray(masks[b]).reshape(-1) > 0.5).astype(np.int64)
        np.add.at(out, (cls, bins), 1)
        near += int((np.abs(f - np.round(f)) < MARGIN * np.maximum(1.0, np.abs(zb)) * (NB / 32.0)).sum())
    return out, near


def auc_from_bins(bins):
    """(AUC, half-width) as heads.MaskMetrics.auc_from_hist defines them, written independently."""
    neg, pos = bins[0].astype(np.float64), bins[1].astype(np.float64)
    P, N = pos.sum(), neg.sum()
    if P == 0 or N == 0:
        return float("nan"), float("nan")
    wins = sum(pos[b] * neg[:b].sum() for b in np.nonzero(pos)[0])
    ties = (pos * neg).sum()
    return float((wins + 0.5 * ties) / (P * N)), float(0.5 * ties / (P * N))


def auc_edge_allowance(bins, near):
    """The most `near` pixels that land in a neighbouring bin can move the AUC: one foreground pixel moved one bin changes the
    pair count by at most half the background pixels of the two bins, and the other way round."""
    neg, pos = bins[0].astype(np.float64), bins[1].astype(np.float64)
    P, N = pos.sum(), neg.sum()
    return float(near * max(neg.max(), pos.max()) / (P * N)) if P and N else 0.0


def pack_masks(masks):
    m = np.asarray(masks)
    assert set(np.unique(m).tolist()) <= {0, 1}
    return np.packbits(m.astype(np.uint8).reshape(-1))


def unpack_masks(packed, B, S):
    return np.unpackbits(packed)[:B * S * S].reshape(B, S, S)


def load_cases():
    """Every golden case as a dict of arrays (plus `name`, `best`, `B`, `g`, `S`)."""
    with open(os.path.join(GOLDEN_DIR, "cases.json")) as f:
        doc = json.load(f)
    out = []
    for meta in doc["cases"]:
        z = np.load(os.path.join(GOLDEN_DIR, meta["name"] + ".npz"))
        case = dict(meta)
        case.update({k: z[k] for k in z.files})
        case["masks"] = unpack_masks(case.pop("masks_packed"), meta["B"], meta["S"])
        case["has_mask"] = np.asarray(meta["has_mask"], dtype=bool)
        out.append(case)
    return doc, out
