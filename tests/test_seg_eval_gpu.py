"""Mask localisation metrics on the GPU (csrc/decoder_tail.hip: seg_eval; head_ops.seg_eval_from_lowres; heads.MaskMetrics)
against the golden data of tests/golden/seg_eval/: float64 pixel counts, the numbers the reference's own
`dice_iou_from_logits` / `sweep_mask_thresholds` produced, and sklearn's AUC.

The count rule.  The kernel forms every up-sampled logit in fp32, the golden counts in float64.  For |z| <= 16 the two differ
by a few ulp(16) = 1.9e-6, under 2^-16 max(1, |z|); only a pixel that close to a cut (a BORDERLINE pixel; the fixtures record
how many each (image, cut) has) can be counted on the other side of it.  So bin k of an image may differ from the golden
count by at most the borderline pixels of the two cuts that bound it, and a metric at cut j by at most what that many
pixels changing sides can do (`*_dev` in the fixtures, seg_eval_ref.curves_from_hist)."""
import numpy as np
import pytest
import torch

import seg_eval_ref as R
from abi_harness import Arena, assert_guards

pytestmark = pytest.mark.gpu
F32, U8 = 0, 6
NB = R.NB


@pytest.fixture(scope="module")
def golden():
    return R.load_cases()


def case_named(golden, name):
    return next(c for c in golden[1] if c["name"] == name)


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def stream():
    return torch.cuda.current_stream().cuda_stream


class Out:
    """hist and auc_hist in guarded arenas: hist poisoned (the call overwrites it), auc_hist zero (the call adds to it)."""

    def __init__(self, B, K, auc=True):
        self.B, self.K = B, K
        self.hist = Arena(B * 2 * (K + 1) * 4, 0xFF)
        self.auc = Arena(2 * NB * 8, 0x00) if auc else None

    def arenas(self):
        return [("hist", self.hist)] + ([("auc_hist", self.auc)] if self.auc else [])

    def hist_np(self):
        return self.hist.payload.view(torch.int32).view(self.B, 2, self.K + 1).cpu().numpy().astype(np.int64)

    def auc_np(self):
        return self.auc.payload.view(torch.int64).view(2, NB).cpu().numpy()


def launch(lib, lr, tgt, cuts, out, sel=None, dt=None):
    """sgl_op_seg_eval on device tensors; the status is asserted, the guards checked after a synchronise."""
    B, g, S = lr.shape[0], lr.shape[-1], tgt.shape[-1]
    dt = (F32 if tgt.dtype == torch.float32 else U8) if dt is None else dt
    st = lib.sgl_op_seg_eval(lr.data_ptr(), tgt.data_ptr(), dt, None if sel is None else sel.data_ptr(), cuts.data_ptr(),
                             cuts.numel(), out.hist.ptr, out.auc.ptr if out.auc else None, B, g, S, stream())
    assert st == 0, st
    torch.cuda.synchronize()
    assert_guards(out.arenas(), "sgl_op_seg_eval")
    return out.hist_np()


def assert_counts(hist, want, border, has_mask, masks, what):
    """The count rule of the module docstring, exact row sums and class totals, zero rows outside the selection."""
    B, _, K1 = want.shape
    S2 = masks[0].size
    slack = np.zeros((B, K1), dtype=np.int64)
    slack[:, :-1] += border                   # bin k is bounded below by cut k-1 and above by cut k
    slack[:, 1:] += border
    for b in range(B):
        if not has_mask[b]:
            assert not hist[b].any(), (what, b)
            continue
        diff = np.abs(hist[b] - want[b])
        assert (diff <= slack[b][None, :]).all(), (what, b, diff.max(), slack[b].max())
        assert hist[b].sum() == S2
        assert hist[b, 1].sum() == int(masks[b].sum()) and hist[b, 0].sum() == S2 - int(masks[b].sum())


@pytest.mark.parametrize("name", ["odd17", "mid96", "base224", "so400m384", "single5"])
def test_counts_match_the_golden_float64_histogram(hiplib, golden, name):
    case = case_named(golden, name)
    lr, cuts, sel = dev(case["lr"]), dev(case["cuts"]), dev(case["has_mask"], torch.uint8)
    out = Out(case["B"], len(case["cuts"]))
    hist = launch(hiplib, lr, dev(case["masks"], torch.float32), cuts, out, sel)
    print(f"{name}: max |count - golden| = {np.abs(hist - case['hist']).max()}, borderline = {int(case['borderline'].sum())}")
    assert_counts(hist, case["hist"], case["borderline"], case["has_mask"], case["masks"], name)
    # the AUC bins hold every selected pixel once, class by class
    bins = out.auc_np()
    assert (bins.sum(1) == case["auc_bins"].sum(1)).all() and (bins >= 0).all()
    # and differ from the float64 bins only where a pixel sits within the margin of a bin edge
    assert np.abs(bins - case["auc_bins"]).sum() <= 2 * int(case["auc_near_edge"])


def test_mask_dtypes_and_selection(pkg, hiplib, golden):
    case = case_named(golden, "mid96")
    B, K = case["B"], len(case["cuts"])
    lr, cuts = dev(case["lr"]), dev(case["cuts"])
    m_f32, m_u8 = dev(case["masks"], torch.float32), dev(case["masks"], torch.uint8)
    sel = dev(case["has_mask"], torch.uint8)
    o_f, o_u = Out(B, K), Out(B, K)
    h_f, h_u = launch(hiplib, lr, m_f32, cuts, o_f, sel), launch(hiplib, lr, m_u8, cuts, o_u, sel)
    assert np.array_equal(h_f, h_u) and np.array_equal(o_f.auc_np(), o_u.auc_np())
    assert not h_f[1].any() and h_f[0].any() and h_f[2].any()            # the image without a mask: a zero row
    o_all, o_ones = Out(B, K), Out(B, K)
    h_all = launch(hiplib, lr, m_u8, cuts, o_all, None)
    h_ones = launch(hiplib, lr, m_u8, cuts, o_ones, torch.ones(B, dtype=torch.uint8, device="cuda"))
    assert np.array_equal(h_all, h_ones) and np.array_equal(o_all.auc_np(), o_ones.auc_np())
    assert np.array_equal(h_all[[0, 2]], h_f[[0, 2]]) and h_all[1].sum() == case["S"] ** 2
    # a soft mask is thresholded at 0.5 (0.5 itself is background), a byte mask at non-zero
    soft = m_f32 * 0.2 + 0.4 - (1 - m_f32) * 0.1                          # foreground 0.6, background 0.3
    soft[0, 0, :5] = 0.5
    ref = m_u8.clone()
    ref[0, 0, :5] = 0
    assert np.array_equal(launch(hiplib, lr, soft, cuts, Out(B, K)), launch(hiplib, lr, ref, cuts, Out(B, K)))
    assert np.array_equal(launch(hiplib, lr, m_u8 * 255, cuts, Out(B, K)), h_all)
    # the Python entry: bool / uint8 / float / half masks, (B,1,S,S) or (B,S,S); half logits are upcast, not re-rounded
    f = pkg.seg_eval_from_lowres
    has = dev(case["has_mask"])
    want = torch.from_numpy(h_f).int().cuda()
    for masks in (m_u8.bool()[:, None], m_u8, m_f32[:, None], m_f32.half(), m_f32.double()):
        assert torch.equal(f(lr[:, None], masks, has, cuts=cuts), want)
    assert torch.equal(f(lr, m_u8, has, cuts=case["cuts"].tolist()), want)                  # host cuts: checked, uploaded
    assert torch.equal(f(lr, m_u8, None, cuts=cuts), torch.from_numpy(h_all).int().cuda())
    for half in (torch.bfloat16, torch.float16):
        lo = lr.to(half)
        assert torch.equal(f(lo, m_u8, has, cuts=cuts), f(lo.float(), m_u8, has, cuts=cuts))
    with pytest.raises(ValueError):
        f(lr, m_u8, has, cuts=[1.0, 0.0])
    with pytest.raises(ValueError):
        f(lr, m_u8.int(), has, cuts=cuts)


@pytest.mark.parametrize("K", [1, 18, 64])
@pytest.mark.parametrize("name", ["odd17", "mid96"])
def test_cut_counts_and_mask_alignments(hiplib, golden, name, K):
    """K = 1, 18 and 64 cuts (the search's shortest and longest paths) against the float64 counts, and the same result from
    masks whose first element sits 0 / 4 / 8 / 12 bytes (fp32) or 0 / 1 / 5 / 15 bytes (bytes) past a 16-byte boundary:
    head, 16-byte body and tail of every band are split differently each time.  odd17 has 17-element rows (every row starts
    at another alignment) and one band; mid96 has a 64-row and a 32-row band per image."""
    case = case_named(golden, name)
    B, S = case["B"], case["S"]
    cuts_np = {1: np.array([0.0], np.float32), 18: case["cuts"], 64: np.linspace(-4.0, 4.0, 64).astype(np.float32)}[K]
    z = R.upsample64(case["lr"], S)
    want, border = R.hist64(z, case["masks"], cuts_np), R.borderline(z, cuts_np)
    lr, cuts = dev(case["lr"]), dev(cuts_np)
    first = None
    for dtype, offsets in ((torch.float32, (0, 1, 2, 3)), (torch.uint8, (0, 1, 5, 15))):
        for off in offsets:
            buf = torch.full((B * S * S + 16,), 77, dtype=dtype, device="cuda")        # 77: neither 0 nor 1 around the view
            view = buf[off:off + B * S * S].view(B, S, S)
            view.copy_(dev(case["masks"], dtype))
            assert view.data_ptr() % 16 == (off * buf.element_size()) % 16
            out = Out(B, K)
            hist = launch(hiplib, lr, view, cuts, out)
            if first is None:
                first = (hist, out.auc_np())
                assert_counts(hist, want, border, np.ones(B, bool), case["masks"], (name, K))
            else:
                assert np.array_equal(hist, first[0]) and np.array_equal(out.auc_np(), first[1]), (dtype, off)


def test_reproducible_and_accumulating(hiplib, golden):
    case = case_named(golden, "so400m384")
    B, K = case["B"], len(case["cuts"])
    lr, cuts, masks = dev(case["lr"]), dev(case["cuts"]), dev(case["masks"], torch.uint8)
    a, b = Out(B, K), Out(B, K)
    assert np.array_equal(launch(hiplib, lr, masks, cuts, a), launch(hiplib, lr, masks, cuts, b))
    assert np.array_equal(a.auc_np(), b.auc_np())
    whole = a.auc_np().copy()
    # hist is overwritten, auc_hist added to: image 0 then image 1 into one pair of arenas
    parts = Out(1, K)
    h0 = launch(hiplib, lr[:1], masks[:1], cuts, parts)
    first = parts.auc_np().copy()
    h1 = launch(hiplib, lr[1:], masks[1:], cuts, parts)
    assert np.array_equal(np.concatenate([h0, h1]), a.hist_np())
    assert np.array_equal(parts.auc_np(), whole) and first.sum() == case["S"] ** 2 and (parts.auc_np() >= first).all()
    launch(hiplib, lr, masks, cuts, a)                                                   # again into `a`: doubled
    assert np.array_equal(a.auc_np(), 2 * whole)
    # selection: an unselected image adds nothing
    sel = Out(B, K)
    launch(hiplib, lr, masks, cuts, sel, torch.tensor([1, 0], dtype=torch.uint8, device="cuda"))
    assert np.array_equal(sel.auc_np(), first)
    # NULL auc_hist: the same hist, and an arena that was not handed over stays as it was
    spare = Arena(2 * NB * 8, 0x5A)
    none = Out(B, K, auc=False)
    assert np.array_equal(launch(hiplib, lr, masks, cuts, none), b.hist_np())
    assert spare.untouched() and spare.guards_intact()


def test_class_totals_agree_with_the_loss_kernel(hiplib, golden):
    case = case_named(golden, "mid96")
    B, g, S, K = case["B"], case["g"], case["S"], len(case["cuts"])
    lr, masks = dev(case["lr"]), dev(case["masks"], torch.float32)
    chunks = hiplib.sgl_op_seg_loss_chunks(S)
    partial = torch.empty(B, chunks, 4, device="cuda")
    assert hiplib.sgl_op_seg_loss_fwd(lr.data_ptr(), masks.data_ptr(), partial.data_ptr(), B, g, S, stream()) == 0
    hist = launch(hiplib, lr, masks, dev(case["cuts"]), Out(B, K))
    sum_t = partial[:, :, 3].double().sum(1).cpu().numpy()
    assert np.array_equal(hist[:, 1].sum(1), sum_t.astype(np.int64)) and (sum_t == np.round(sum_t)).all()
    assert np.array_equal(hist.sum((1, 2)), np.full(B, S * S))


def sync_debug_is_honoured():
    """Whether this build raises on a synchronising call under set_sync_debug_mode("error")."""
    x = torch.ones(1, device="cuda")
    torch.cuda.set_sync_debug_mode("error")
    try:
        x.item()
    except RuntimeError:
        return True
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return False


@pytest.mark.parametrize("mask_thr", [0.5, 0.37])
def test_mask_metrics_end_to_end(pkg, hiplib, golden, mask_thr):
    """MaskMetrics.update over every fixture in two batches: the reference's curves within what the borderline pixels allow
    (+1e-6 for its fp32 `.tolist()`), its best thresholds exactly, sklearn's AUC within the golden half-width; no update
    synchronises with the host."""
    doc, cases = golden
    at = doc["extra_thresholds"].index(mask_thr)
    honoured = sync_debug_is_honoured()
    print(f"set_sync_debug_mode('error') honoured: {honoured}")
    for case in cases:
        B = case["B"]
        lr, masks, has = dev(case["lr"])[:, None], dev(case["masks"], torch.uint8)[:, None], dev(case["has_mask"])
        m = pkg.MaskMetrics(mask_thr=mask_thr)
        half = max(1, B // 2)
        torch.cuda.synchronize()
        if honoured:
            torch.cuda.set_sync_debug_mode("error")
        try:
            m.update(lr[:half], masks[:half], has[:half])
            if half < B:
                m.update(lr[half:], masks[half:].float(), has[half:])
        finally:
            torch.cuda.set_sync_debug_mode("default")
        out = m.compute()
        idx = case["sweep_index"]
        for key in ("f1", "dice", "iou"):
            err = np.abs(np.asarray(out[key + "_curve"]) - case["ref_" + key])
            print(f"{case['name']} {key}: max err {err.max():.3e}, allowed {case[key + '_dev'][idx].max() + 1e-6:.3e}")
            assert (err <= case[key + "_dev"][idx] + 1e-6).all(), (case["name"], key)
        j = int(case["extra_index"][at])
        assert abs(out["dice"] - case["ref_dice_at"][at]) <= case["dice_dev"][j] + 1e-6
        assert abs(out["iou"] - case["ref_iou_at"][at]) <= case["iou_dev"][j] + 1e-6
        for key in ("f1", "dice", "iou"):
            assert out["best"]["thr_" + key] == case["best"]["thr_" + key], (case["name"], key)
            k = int(np.argmin(np.abs(np.linspace(0.1, 0.9, 17) - case["best"]["thr_" + key])))
            assert abs(out["best"][key] - case["best"][key]) <= case[key + "_dev"][idx[k]] + 1e-6
        assert out["num_images"] == int(case["has_mask"].sum())
        # AUC over all pixels: within the half-width computed from the GOLDEN bins, plus the pixels near a bin edge
        _, hw = R.auc_from_bins(case["auc_bins"])
        allow = hw + R.auc_edge_allowance(case["auc_bins"], int(case["auc_near_edge"]))
        print(f"{case['name']} auc {out['pix_auc']:.6f} sklearn {float(case['auc_sklearn']):.6f} allowed {allow:.2e}")
        assert abs(out["pix_auc"] - float(case["auc_sklearn"])) <= allow
        assert abs(out["pix_auc_halfwidth"] - hw) <= R.auc_edge_allowance(case["auc_bins"], int(case["auc_near_edge"]))


def test_siglip2mtl_lowres_path_equals_full_resolution_reference(pkg, hiplib):
    """forward(..., return_lowres=True) -> MaskMetrics against forward() (the (B,1,S,S) logits) -> float64 reference on the
    same weights, under the count rule (borderline pixels taken from the full-resolution logits themselves)."""
    H = pkg.heads
    cfg = pkg.get_config("hostile")
    enc = pkg.SiglipVisionModelHIP(cfg, compute_dtype="fp32")
    enc.load_state_dict(pkg.weights.seeded_state_dict(cfg, seed=13))
    torch.manual_seed(0)
    model = H.SigLIP2MTL(enc, seg_layers=(0, 1, -1), embed_dim=32, freeze_below=1).cuda().eval()
    x = pkg.weights.seeded_pixels(3, 56, 56, seed=17).cuda()
    masks = (pkg.weights.seeded_tensor("masks", (3, 1, 56, 56), 1.0) > 0.2).float().cuda()
    has = torch.tensor([True, False, True]).cuda()
    m = H.MaskMetrics()
    with torch.no_grad():
        _, probe = model(x, return_lowres=True)                    # the 1x1 head is affine: rescale and shift it so that
        k = 2.0 / probe.std()                                      # the logits have mean 0 and standard deviation 2 and
        model.decoder.head.weight.mul_(k)                          # cross several cuts
        model.decoder.head.bias.copy_(k * (model.decoder.head.bias - probe.mean()))
        _, seg = model(x)
        _, seg_lr = model(x, return_lowres=True)
        hist = pkg.seg_eval_from_lowres(seg_lr, masks, has, cuts=m.device_cuts("cuda:0")).cpu().numpy().astype(np.int64)
        m.update(seg_lr, masks, has)
    assert seg.shape == (3, 1, 56, 56) and seg_lr.shape == (3, 1, 4, 4)
    z = seg[:, 0].double().cpu().numpy()
    mk, hm = masks[:, 0].cpu().numpy(), has.cpu().numpy()
    assert np.abs(z).max() <= 16 and np.unique(np.searchsorted(m.cuts.astype(np.float64), z[hm])).size >= 4
    want, border = R.hist64(z, mk, m.cuts, hm), R.borderline(z, m.cuts, hm)
    assert_counts(hist, want, border, hm, mk, "SigLIP2MTL")
    cur = R.curves_from_hist(want, hm, border)
    out = m.compute()
    for key in ("f1", "dice", "iou"):
        assert (np.abs(np.asarray(out[key + "_curve"]) - cur[key][m.sweep_index]) <= cur[key + "_dev"][m.sweep_index] + 1e-12).all()
    assert out["num_images"] == 2
