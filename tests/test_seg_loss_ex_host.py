"""CPU (no GPU): the float64 reference of sgl_op_seg_loss_ex_fwd / _bwd (tests/seg_loss_ex_ref.py) is
`heads.combined_segmentation_loss` of the bilinearly up-sampled logits and its autograd; the fp32 emulation of the kernels'
arithmetic stays inside the derived bounds and four mutants leave them; the entry points' refusals, the wrapper's `terms`
mask and CPU error, and `training_loss`'s new keywords.  No kernel is launched here."""
import inspect

import pytest
import torch

import kernel_ref as kr
import seg_loss_ex_ref as sr

F = torch.nn.functional
OK, BAD_SHAPE, UNSUPPORTED, NULL = 0, -1, -2, -5
D = 0x7F0000001000          # a 16-byte aligned dummy device pointer, never dereferenced
WEIGHTS = dict(bce_w=0.4, focal_w=0.3, dice_w=0.5, boundary_w=0.4, iou_w=0.4, morph_w=0.2)
ALL = sr.FOCAL | sr.BOUNDARY | sr.TV
CASE_SETS = [(case, k) for case in sr.CASES for k in sr.mask_sets(case[0])]


@pytest.fixture(scope="module")
def alpha(pkg, hiplib):
    """The focal alpha the wrapper hands the kernels; the reference and the emulation are exercised with it and with the
    package's own term bits, so this module stands or falls with the entry points it describes."""
    assert hasattr(hiplib, "sgl_op_seg_loss_ex_fwd") and hasattr(hiplib, "sgl_op_seg_loss_ex_bwd")
    assert (pkg.lib.SEG_TERM_FOCAL, pkg.lib.SEG_TERM_BOUNDARY, pkg.lib.SEG_TERM_TV) == (sr.FOCAL, sr.BOUNDARY, sr.TV)
    assert pkg.head_ops._FOCAL_ALPHA == inspect.signature(pkg.heads.focal_loss).parameters["alpha"].default
    return pkg.head_ops._FOCAL_ALPHA


def loss_of_sums(sums, S, w):
    """The wrapper's composition of the folded sums [B, 8] (every image selected), float64."""
    s, B = sums.double(), sums.shape[0]
    N, pairs = B * S * S, B * S * (S - 1)
    I, P, T = s[:, 1], s[:, 2], s[:, 3]
    dice = 1 - (2 * I / (P + T + 1e-6)).mean()
    iou = 1 - (I / (P + T - I + 1e-6)).mean()
    return (w["bce_w"] * s[:, 0].sum() / N + w["focal_w"] * s[:, 4].sum() / N + w["dice_w"] * dice
            + w["boundary_w"] * s[:, 5].sum() / N + w["iou_w"] * iou + w["morph_w"] * (s[:, 6] + s[:, 7]).sum() / pairs)


def coef_of(B, S, w, up=1.0):
    N, pairs = float(B * S * S), float(B * S * (S - 1))
    row = [up * w["bce_w"] / N, -up * w["dice_w"] / B, up * w["focal_w"] / N, up * w["boundary_w"] / N,
           -up * w["iou_w"] / B, up * w["morph_w"] / pairs]
    return torch.tensor([row] * B, dtype=torch.float64)


@pytest.mark.parametrize("case,mask_set", CASE_SETS, ids=str)
def test_reference_is_combined_segmentation_loss_and_its_autograd(pkg, alpha, case, mask_set):
    """Loss and d loss / d low-res logits of the reference against float64 autograd of F.interpolate(bilinear,
    align_corners=False) -> heads.combined_segmentation_loss.  The reference places its taps with the kernel's fp32 scale
    fl(g) / fl(S), torch with the double: positions differ by 2^-24 g (the position term `cs` of the bound), values by that
    times the slope.  The smooth part of the difference is held to the tolerances of
    test_seg_loss_reference_is_interpolate_bce_dice_and_bound_holds; a pair of neighbours whose p differ by no more than
    the position term (the clamped last rows / columns, where torch's l (1 - w) + l w rounds either way, among them) may
    have either sign in torch: 2 |c_tv| p (1 - p) per such pair, spread by the bilinear weights."""
    B, g, S = case
    H = pkg.heads
    lr, tgt, _ = sr.inputs(B, g, S, mask_set)
    r = sr.pixels(lr, tgt, alpha)
    ref, _ = sr.seg_loss_ex_fwd_ref(lr, tgt, r=r)
    L = lr.double().requires_grad_(True)
    up = F.interpolate(L[:, None], size=(S, S), mode="bilinear", align_corners=False)
    want = H.combined_segmentation_loss(up, tgt.double()[:, None])
    want.backward()
    sums64 = ref.sum(1)
    got = loss_of_sums(sums64, S, WEIGHTS)
    assert abs(got.item() - want.item()) <= 1e-6 * abs(want.item()) + 1e-9, (got.item(), want.item())
    coef = coef_of(B, S, WEIGHTS)
    # float64 sums / coef: the reference's formula itself, no fp32 rounding of its operands
    W = r["W"]
    dz, _ = sr.pixel_grad_ref(r, sums64, coef, ALL, 1e-6, 1e-6)
    dref = W.t() @ dz @ W
    epos = r["p"] * (1 - r["p"]) * r["cs"] * ((r["Dm"] @ lr.double() @ W.t()).abs() + (W @ lr.double() @ r["Dm"].t()).abs()) \
        + 1e-14
    amb_x = (r["dx"].abs() <= epos[:, :, 1:] + epos[:, :, :-1]).double()
    amb_y = (r["dy"].abs() <= epos[:, 1:, :] + epos[:, :-1, :]).double()
    namb = sr._neighbour_sum(amb_x, amb_y, torch.abs)
    sign_tol = W.t() @ (2 * coef[:, 5, None, None].abs() * r["p"] * (1 - r["p"]) * namb) @ W
    tol = 1e-4 * L.grad.abs() + 1e-5 * L.grad.abs().max() + sign_tol
    assert ((dref - L.grad).abs() <= tol).all(), ((dref - L.grad).abs() / tol).max().item()
    # outside the identical rows the allowance is rare: it cannot carry a wrong formula
    live = max(1, int((~r["same"]).sum())) * S * B
    assert (amb_x[:, :, ~r["same"]].sum() + amb_y[:, ~r["same"], :].sum()) / (2 * live) <= sr.MAX_AMBIGUOUS_SHARE


@pytest.mark.parametrize("case,mask_set", CASE_SETS, ids=str)
def test_emulation_within_bounds_and_ambiguous_pairs_rare(alpha, case, mask_set):
    """The fp32 emulation against the element-wise bounds (every `terms` mask at the first shape, the full mask elsewhere),
    unselected sums exact zeros, and at most 0.2 % of the non-identical neighbour pairs ambiguous per axis."""
    B, g, S = case
    lr, tgt, coef = sr.inputs(B, g, S, mask_set)
    r = sr.pixels(lr, tgt, alpha)
    ax, ay = sr.ambiguous_share(r)
    print(f"AMBIGUOUS {case} set {mask_set}: x {ax:.5f} y {ay:.5f}")
    assert ax <= sr.MAX_AMBIGUOUS_SHARE and ay <= sr.MAX_AMBIGUOUS_SHARE, (ax, ay)
    worst = 0.0
    for terms in (range(8) if case == sr.CASES[0] else (ALL,)):
        ref, bound = sr.seg_loss_ex_fwd_ref(lr, tgt, terms=terms, r=r)
        sums = sr.fold(ref)
        dref, dbound = sr.seg_loss_ex_bwd_ref(lr, tgt, sums, coef, terms=terms, r=r)
        part, dlr = sr.emulate(lr, tgt, sums, coef, alpha, terms=terms)
        worst = max(worst, kr.assert_within(part, ref, bound, f"partials terms={terms}"),
                    kr.assert_within(dlr, dref, dbound, f"dlogits_lr terms={terms}"))
        for k, bit in ((4, sr.FOCAL), (5, sr.BOUNDARY), (6, sr.TV), (7, sr.TV)):
            if not terms & bit:
                assert bool((ref[..., k] == 0).all()) and bool((bound[..., k] == 0).all())
    print(f"RATIO seg_loss_ex emulation {case} set {mask_set}: {worst:.4f}")
    assert worst <= 0.5, worst
    if g == 1:       # all taps coincide: the smoothness sums are exact zeros in the reference and in the emulation
        assert bool((ref[..., 6:] == 0).all()) and bool((part[..., 6:] == 0).all())


@pytest.mark.parametrize("mutant", sr.MUTANTS)
def test_mutants_leave_the_bounds(alpha, mutant):
    """Each mutant of seg_loss_ex_ref.emulate exceeds a bound at (2, 3, 42), on the rectangle + island / noise masks and
    on the all-ones / all-zeros masks taken together."""
    B, g, S = sr.CASES[0]
    worst = 0.0
    for mask_set in sr.mask_sets(B):
        lr, tgt, coef = sr.inputs(B, g, S, mask_set)
        r = sr.pixels(lr, tgt, alpha)
        ref, bound = sr.seg_loss_ex_fwd_ref(lr, tgt, r=r)
        sums = sr.fold(ref)
        dref, dbound = sr.seg_loss_ex_bwd_ref(lr, tgt, sums, coef, r=r)
        part, dlr = sr.emulate(lr, tgt, sums, coef, alpha, mutant=mutant)
        worst = max(worst, kr.worst_ratio(part, ref, bound), kr.worst_ratio(dlr, dref, dbound))
    assert worst > 10, (mutant, worst)


def test_entry_points_refuse_null_and_bad_shapes(pkg, hiplib):
    lib = hiplib
    assert hiplib.sgl_abi_version() == 3
    assert {"sgl_op_seg_loss_ex_fwd", "sgl_op_seg_loss_ex_bwd"} <= set(pkg.lib.declared_symbols())
    fwd = lambda a, b, g, s, terms=7: lib.sgl_op_seg_loss_ex_fwd(*a, b, g, s, terms, 0.25, None)
    bwd = lambda a, b, g, s, terms=7: lib.sgl_op_seg_loss_ex_bwd(*a, b, g, s, terms, 0.25, 1e-6, 1e-6, None)
    for b, g, s in ((0, 3, 42), (-1, 3, 42), (1, 0, 42), (1, 3, 0), (1, 3, 1), (1, 4097, 42), (1, 3, 2049)):
        assert fwd([D] * 3, b, g, s) == BAD_SHAPE, (b, g, s)
        assert bwd([D] * 5, b, g, s) == BAD_SHAPE, (b, g, s)
    for terms in (8, -1, 15):
        assert fwd([D] * 3, 1, 3, 42, terms) == UNSUPPORTED and bwd([D] * 5, 1, 3, 42, terms) == UNSUPPORTED
    for k in range(3):
        a = [D] * 3
        a[k] = None
        assert fwd(a, 1, 3, 42) == NULL
    for k in range(5):
        a = [D] * 5
        a[k] = None
        assert bwd(a, 1, 3, 42) == NULL


def test_wrapper_terms_mask_cpu_error_and_training_loss_keywords(pkg):
    ho, H, Lb = pkg.head_ops, pkg.heads, pkg.lib
    assert (Lb.SEG_TERM_FOCAL, Lb.SEG_TERM_BOUNDARY, Lb.SEG_TERM_TV) == (sr.FOCAL, sr.BOUNDARY, sr.TV)
    for terms in range(8):
        fw, bw, mw = (0.3 if terms & sr.FOCAL else 0.0, 0.4 if terms & sr.BOUNDARY else 0.0, 0.2 if terms & sr.TV else 0.0)
        assert ho.seg_terms_mask(fw, bw, mw) == terms
    assert ho.seg_terms_mask(-0.1, 0.0, 1e-30) == sr.FOCAL | sr.TV
    assert H.combined_loss_from_lowres is ho.combined_loss_from_lowres
    sig = inspect.signature(ho.combined_loss_from_lowres)
    want = inspect.signature(H.combined_segmentation_loss)
    for k in ("bce_w", "focal_w", "dice_w", "boundary_w", "iou_w", "morph_w", "eps"):
        assert sig.parameters[k].default == want.parameters[k].default, k
    assert sig.parameters["smooth"].default == inspect.signature(H.iou_loss).parameters["smooth"].default
    assert sig.parameters["has_mask"].default is None
    with pytest.raises(RuntimeError, match="combined_segmentation_loss"):
        ho.combined_loss_from_lowres(torch.zeros(1, 1, 3, 3), torch.zeros(1, 1, 6, 6))
    tl = inspect.signature(H.SigLIP2MTL.training_loss).parameters
    assert [tl[k].default for k in ("enhanced", "focal_w", "boundary_w", "iou_w", "morph_w")] == [False, 0.3, 0.4, 0.4, 0.2]
    assert [tl[k].default for k in ("lam_seg", "bce_w", "dice_w")] == [1.0, 1.0, 0.5]
