"""CPU (no GPU): the mask localisation metrics' C entry point (argument checks only: every call returns before a HIP call,
as in tests/test_abi_aux_host.py) and `heads.MaskMetrics` on CPU tensors, fed the golden float64 pixel counts of
tests/golden/seg_eval/ (made by tests/gen_golden_seg_eval.py, which ran the reference's own `dice_iou_from_logits` and
`sweep_mask_thresholds`)."""
import math
import re

import numpy as np
import pytest
import torch

import seg_eval_ref as R

OK, BAD_SHAPE, UNSUPPORTED, NULL = 0, -1, -2, -5
D = 0x7F0000001000          # a 16-byte aligned dummy device pointer, never dereferenced
F32, U8 = 0, 6
TOL = 1e-6                  # the reference's numbers went through fp32 `.tolist()`


@pytest.fixture(scope="module")
def golden():
    return R.load_cases()


def drop_cut(hist, j):
    """The counts without cut j: the bins on either side of it merge."""
    h = np.asarray(hist)
    return np.concatenate([h[..., :j], h[..., j:j + 1] + h[..., j + 1:j + 2], h[..., j + 2:]], axis=-1)


def test_symbols_are_declared_exported_and_the_abi_version_stays(pkg, hiplib):
    declared = pkg.lib.declared_symbols()
    for name in ("sgl_op_seg_eval", "sgl_op_seg_eval_auc_bins"):
        assert name in declared and hasattr(hiplib, name)
    assert hiplib.sgl_abi_version() == 3
    with open(pkg.lib.HEADER_PATH) as f:
        text = f.read()
    assert int(re.search(r"#define\s+SGL_SEG_EVAL_AUC_BINS\s+(\d+)", text).group(1)) == 4096
    assert hiplib.sgl_op_seg_eval_auc_bins() == pkg.lib.SEG_EVAL_AUC_BINS == R.NB == 4096
    assert re.search(r"SGL_DTYPE_U8\s*=\s*6\b", text) and pkg.lib.SGL_DTYPE_U8 == U8
    assert pkg.MaskMetrics is pkg.heads.MaskMetrics and pkg.seg_eval_from_lowres is pkg.head_ops.seg_eval_from_lowres


def test_every_refusal_comes_before_a_launch(hiplib):
    def call(lr=D, tgt=D, dt=F32, sel=D, cuts=D, K=18, hist=D, auc=D, B=2, g=3, S=17):
        return hiplib.sgl_op_seg_eval(lr, tgt, dt, sel, cuts, K, hist, auc, B, g, S, None)
    for name in ("lr", "tgt", "cuts", "hist"):
        assert call(**{name: None}) == NULL
        assert call(**{name: None}, B=0) == NULL                 # a NULL pointer is reported first
    for bad in (dict(B=0), dict(g=0), dict(S=0), dict(B=-1), dict(g=-3), dict(S=-17), dict(K=0), dict(K=-1), dict(K=65),
                dict(S=32769), dict(S=1 << 30), dict(g=32769)):
        assert call(**bad) == BAD_SHAPE
        assert call(**bad, dt=U8, sel=None, auc=None) == BAD_SHAPE
    for dt in (1, 2, 3, 4, 5, 7, -1):
        assert call(dt=dt) == UNSUPPORTED
    for off in (1, 2, 3):
        assert call(tgt=D + off) == BAD_SHAPE                    # fp32 targets off their natural alignment


def test_cut_order_is_checked_in_python(pkg):
    check = pkg.head_ops.check_cuts
    check([-1.0, 0.0, 2.5])
    check([0.0])
    for bad in ([], [0.0, 0.0], [1.0, -1.0], [0.0, float("nan")], list(range(65))):
        with pytest.raises(ValueError):
            check(bad)
    with pytest.raises(RuntimeError, match="GPU"):
        pkg.seg_eval_from_lowres(torch.zeros(1, 1, 2, 2), torch.zeros(1, 1, 4, 4), cuts=[0.0])


def test_cuts_are_the_fp32_logits_of_the_fp32_thresholds(pkg, golden):
    m = pkg.MaskMetrics(mask_thr=0.37)
    _, cases = golden
    assert m.cuts.dtype == np.float32 and np.array_equal(m.cuts, cases[0]["cuts"])
    assert np.array_equal(m.sweep_index, cases[0]["sweep_index"]) and m.mask_index == cases[0]["extra_index"][1]
    m = pkg.MaskMetrics()                                        # 0.5 is the ninth sweep threshold: no extra cut
    assert len(m.cuts) == 17 and m.mask_index == 8 and m.cuts[8] == 0.0
    for thr, cut in zip(m.sweep_thresholds, m.cuts):
        t = np.float64(np.float32(thr))
        assert cut == np.float32(math.log(t / (1.0 - t)))


@pytest.mark.parametrize("mask_thr", [0.5, 0.37])
def test_compute_from_the_golden_counts_reproduces_the_reference(pkg, golden, mask_thr):
    doc, cases = golden
    assert len(cases) == 5
    for case in cases:
        hist = case["hist"]
        at = doc["extra_thresholds"].index(mask_thr)
        if mask_thr == 0.5:
            hist = drop_cut(hist, int(case["extra_index"][1]))    # the 0.37 cut is not one of this accumulator's
        m = pkg.MaskMetrics(mask_thr=mask_thr)
        m.update_from_hist(torch.from_numpy(hist).double(), torch.from_numpy(case["has_mask"]))
        out = m.compute()
        assert out["num_images"] == int(case["has_mask"].sum())
        for key in ("f1", "dice", "iou"):
            err = np.abs(np.asarray(out[key + "_curve"]) - case["ref_" + key]).max()
            assert err <= TOL, (case["name"], key, err)
        assert abs(out["dice"] - case["ref_dice_at"][at]) <= TOL and abs(out["iou"] - case["ref_iou_at"][at]) <= TOL
        for key, want in case["best"].items():
            assert abs(out["best"][key] - want) <= TOL, (case["name"], key, out["best"][key], want)
        assert np.allclose(out["thresholds"], np.linspace(0.1, 0.9, 17), rtol=0, atol=0)


def test_auc_from_bins_matches_sklearn_within_its_own_half_width(pkg, golden):
    _, cases = golden
    for case in cases:
        auc, hw = pkg.MaskMetrics.auc_from_hist(case["auc_bins"])
        ref_auc, ref_hw = R.auc_from_bins(case["auc_bins"])
        assert abs(auc - ref_auc) <= 1e-12 and abs(hw - ref_hw) <= 1e-15
        assert abs(auc - float(case["auc_sklearn"])) <= hw, (case["name"], auc, float(case["auc_sklearn"]), hw)
        m = pkg.MaskMetrics()
        m.update_from_hist(torch.from_numpy(drop_cut(case["hist"], int(case["extra_index"][1]))),
                           torch.from_numpy(case["has_mask"]), auc_hist=torch.from_numpy(case["auc_bins"]))
        out = m.compute()
        assert out["pix_auc"] == auc and out["pix_auc_halfwidth"] == hw


def test_merge_of_two_halves_equals_the_whole_bit_for_bit(pkg, golden):
    _, cases = golden
    case = next(c for c in cases if c["name"] == "mid96")
    hist, has = torch.from_numpy(case["hist"]), torch.from_numpy(case["has_mask"])
    bins = torch.from_numpy(case["auc_bins"])
    whole = pkg.MaskMetrics(mask_thr=0.37).update_from_hist(hist[:1], has[:1], auc_hist=bins // 2)        # one accumulator,
    whole.update_from_hist(hist[1:], has[1:], auc_hist=bins - bins // 2)                                  # both halves
    once = pkg.MaskMetrics(mask_thr=0.37).update_from_hist(hist, has, auc_hist=bins).state()
    for key, t in whole.state().items():            # against one update of everything: integers exact, float64 sums to an ulp
        assert torch.equal(once[key], t) if t.dtype == torch.int64 else (once[key] - t).abs().max() <= 1e-15 * 3, key
    a = pkg.MaskMetrics(mask_thr=0.37).update_from_hist(hist[:1], has[:1], auc_hist=bins // 2)
    b = pkg.MaskMetrics(mask_thr=0.37).update_from_hist(hist[1:], has[1:], auc_hist=bins - bins // 2)
    a.merge(b)
    empty = pkg.MaskMetrics(mask_thr=0.37)
    a.merge(empty)                                               # nothing accumulated: adds nothing
    for key, t in whole.state().items():
        assert torch.equal(a.state()[key], t), key
    assert a.compute() == whole.compute()
    c = pkg.MaskMetrics(mask_thr=0.37).load_state(whole.state())
    assert c.compute() == whole.compute()
    c.update_from_hist(hist[:1])                                 # a loaded state is a copy
    assert not torch.equal(c.state()["tp"], whole.state()["tp"])
    with pytest.raises(ValueError):
        a.merge(pkg.MaskMetrics())                               # other thresholds
    # data-parallel use: every tensor of state() is additive
    summed = {k: a.state()[k] + whole.state()[k] for k in pkg.MaskMetrics.STATE_KEYS}
    twice = pkg.MaskMetrics(mask_thr=0.37).load_state(whole.state()).merge(whole)
    assert all(torch.equal(summed[k], twice.state()[k]) for k in summed)


def test_unsorted_and_duplicate_thresholds(pkg, golden):
    _, cases = golden
    case = next(c for c in cases if c["name"] == "base224")
    hist = torch.from_numpy(drop_cut(case["hist"], int(case["extra_index"][1])))
    has = torch.from_numpy(case["has_mask"])
    up = pkg.MaskMetrics().update_from_hist(hist, has).compute()
    down_m = pkg.MaskMetrics(thr_min=0.9, thr_max=0.1)           # a descending sweep: same cuts, scanned the other way
    assert np.array_equal(down_m.cuts, pkg.MaskMetrics().cuts) and list(down_m.sweep_index) == list(range(16, -1, -1))
    down = down_m.update_from_hist(hist, has).compute()
    assert down["dice_curve"] == up["dice_curve"][::-1] and down["f1_curve"] == up["f1_curve"][::-1]
    assert down["best"]["dice"] == up["best"]["dice"] and abs(down["best"]["thr_dice"] - up["best"]["thr_dice"]) < 1e-12
    same = pkg.MaskMetrics(thr_min=0.5, thr_max=0.5, thr_steps=4, mask_thr=0.5)       # five thresholds, one cut
    assert len(same.cuts) == 1 and list(same.sweep_index) == [0, 0, 0, 0] and same.mask_index == 0
    h1 = torch.stack([hist[..., :9].sum(-1), hist[..., 9:].sum(-1)], dim=-1)          # only the cut at logit 0 (index 8)
    out = same.update_from_hist(h1, has).compute()
    assert out["dice_curve"] == [up["dice_curve"][8]] * 4 and out["dice"] == up["dice"]
    assert out["best"]["thr_dice"] == 0.5 and out["best"]["dice"] == up["dice_curve"][8]
    for bad in (dict(thr_min=0.0), dict(thr_max=1.0), dict(mask_thr=1.5), dict(thr_steps=70)):
        with pytest.raises(ValueError):
            pkg.MaskMetrics(**bad)


def test_reference_edge_rules(pkg):
    K = 17
    m = pkg.MaskMetrics()
    hist = torch.zeros(2, 2, K + 1, dtype=torch.int32)
    hist[0, 0, 3], hist[0, 0, 12], hist[1, 0, 9] = 50, 50, 100   # background pixels only
    out = m.update_from_hist(hist).compute()
    assert out["f1_curve"] == [0.0] * K and out["best"]["f1"] == 0 and out["best"]["thr_f1"] == 0.5
    assert out["dice_curve"] == [0.0] * K and out["best"]["dice"] == 0 and out["best"]["thr_dice"] == 0.5
    assert math.isnan(out["pix_auc"]) and math.isnan(out["pix_auc_halfwidth"])        # no foreground: nan (:1101)
    m = pkg.MaskMetrics()
    hist = torch.zeros(1, 2, K + 1, dtype=torch.int32)
    hist[0, 1, K] = 64                                           # foreground only, all predicted
    out = m.update_from_hist(hist).compute()
    assert out["f1_curve"] == [0.0] * K                          # masks all one value: f1 = 0 (:220-223)
    assert all(abs(v - 1.0) < 1e-7 for v in out["dice_curve"]) and out["best"]["thr_dice"] == pytest.approx(0.1)
    empty = pkg.MaskMetrics().compute()                          # no update at all
    assert empty["dice"] == 0.0 and empty["iou"] == 0.0 and empty["num_images"] == 0 and math.isnan(empty["pix_auc"])
    assert empty["best"] == {"f1": 0, "dice": 0, "iou": 0, "thr_f1": 0.5, "thr_dice": 0.5, "thr_iou": 0.5}
    # an image outside has_mask adds nothing, whatever its row holds
    a = pkg.MaskMetrics().update_from_hist(torch.randint(0, 9, (3, 2, K + 1)), torch.tensor([True, False, True]))
    h = torch.randint(0, 9, (3, 2, K + 1))
    b = pkg.MaskMetrics().update_from_hist(h, torch.tensor([True, False, True]))
    h[1] = 7
    c = pkg.MaskMetrics().update_from_hist(h, torch.tensor([True, False, True]))
    drop_auc = lambda d: {k: v for k, v in d.items() if not k.startswith("pix_auc")}          # nan here: no AUC bins given
    assert drop_auc(b.compute()) == drop_auc(c.compute()) and a.compute()["num_images"] == 2
    with pytest.raises(ValueError):
        pkg.MaskMetrics().update_from_hist(torch.zeros(1, 2, K))
