"""GPU: sgl_op_seg_loss_ex_fwd / _bwd (csrc/decoder_tail.hip) through the raw C ABI with guarded, poisoned arenas, every
output element held to the bounds of tests/seg_loss_ex_ref.py; `combined_loss_from_lowres` against the float64 composition
with the bounds propagated; `SigLIP2MTL.training_loss(enhanced=True)` against forward() + combined_segmentation_loss."""
import functools

import pytest
import torch

import kernel_ref as kr
import seg_loss_ex_ref as sr
from abi_harness import Arena, stream
from kernel_ref import EPS32

pytestmark = pytest.mark.gpu
F = torch.nn.functional
DEV = "cuda"
OK, BAD_SHAPE, UNSUPPORTED, NULL = 0, -1, -2, -5
ALL = sr.FOCAL | sr.BOUNDARY | sr.TV
CASE_SETS = [(case, k) for case in sr.CASES for k in sr.mask_sets(case[0])]
DEFAULTS = dict(bce_w=0.4, focal_w=0.3, dice_w=0.5, boundary_w=0.4, iou_w=0.4, morph_w=0.2)
# Siglip2sidafrozen.py:1343-1351,1752-1759 with the script's defaults: bce 0.2 * 0.7, dice 0.3 * 0.8, iou min(1.5, 1.5 * 1.5)
IOU_FOCUSED = dict(bce_w=0.14, focal_w=0.0, dice_w=0.24, boundary_w=0.0, iou_w=1.5, morph_w=0.0)


@pytest.fixture(scope="module")
def lib(hiplib):
    assert torch.cuda.is_available()
    return hiplib


@functools.lru_cache(maxsize=None)
def case_ref(case, mask_set, dtype=torch.float32):
    """Inputs and the per-pixel reference of one case, computed once and shared (never modified)."""
    B, g, S = case
    lr, tgt, coef = sr.inputs(B, g, S, mask_set)
    lr = lr.to(dtype).float()
    return lr, tgt, coef, sr.pixels(lr, tgt)


def raw_fwd(lib, lrd, td, B, g, S, terms, alpha=sr.ALPHA):
    chunks = lib.sgl_op_seg_loss_chunks(S)
    part = Arena(B * chunks * 8 * 4, 0xFF, DEV)
    assert lib.sgl_op_seg_loss_ex_fwd(lrd.data_ptr(), td.data_ptr(), part.ptr, B, g, S, terms, alpha, stream()) == OK
    torch.cuda.synchronize()
    assert part.guards_intact(), "seg_loss_ex_fwd wrote outside partial"
    return part.f32(B, chunks, 8).clone()


def raw_bwd(lib, lrd, td, sums, cd, B, g, S, terms, alpha=sr.ALPHA, eps=1e-6, smooth=1e-6):
    dl = Arena(B * g * g * 4, 0xFF, DEV)
    assert lib.sgl_op_seg_loss_ex_bwd(lrd.data_ptr(), td.data_ptr(), sums.data_ptr(), cd.data_ptr(), dl.ptr, B, g, S, terms,
                                      alpha, eps, smooth, stream()) == OK
    torch.cuda.synchronize()
    assert dl.guards_intact(), "seg_loss_ex_bwd wrote outside dlogits_lr"
    return dl.f32(B, g, g).clone()


@pytest.mark.parametrize("case,mask_set", CASE_SETS, ids=str)
def test_raw_abi_within_bounds(lib, case, mask_set):
    """Partial sums and dlogits_lr within their element-wise bounds, guard bands untouched, unselected sums exact zeros,
    two launches bit-equal: every `terms` mask at the first shape, the full mask elsewhere.  With g = 1 all taps coincide
    and the smoothness sums are exact zeros."""
    B, g, S = case
    lr, tgt, coef, r = case_ref(case, mask_set)
    lrd, td, cd = lr.to(DEV), tgt.to(DEV), coef.to(DEV)
    for terms in (range(8) if case == sr.CASES[0] else (ALL,)):
        what = f"seg_loss_ex {case} set {mask_set} terms {terms}"
        part = raw_fwd(lib, lrd, td, B, g, S, terms)
        assert torch.equal(part, raw_fwd(lib, lrd, td, B, g, S, terms)), f"{what}: forward not bitwise reproducible"
        ref, bound = sr.seg_loss_ex_fwd_ref(lr, tgt, terms=terms, r=r)
        rf = kr.assert_within(part.cpu(), ref, bound, what + " partial")
        for k, bit in ((4, sr.FOCAL), (5, sr.BOUNDARY), (6, sr.TV), (7, sr.TV)):
            if not terms & bit:
                assert bool((part[..., k] == 0).all()), f"{what}: sum {k} of an unselected term is not 0"
        if g == 1:
            assert bool((part[..., 6:] == 0).all()), f"{what}: coinciding taps must give exactly zero smoothness sums"
        sums = sr.fold(part.cpu())
        sd = sums.to(DEV)
        dl = raw_bwd(lib, lrd, td, sd, cd, B, g, S, terms)
        assert torch.equal(dl, raw_bwd(lib, lrd, td, sd, cd, B, g, S, terms)), f"{what}: backward not bitwise reproducible"
        dref, dbound = sr.seg_loss_ex_bwd_ref(lr, tgt, sums, coef, terms=terms, r=r)
        rb = kr.assert_within(dl.cpu(), dref, dbound, what + " dlogits_lr")
        print(f"RATIO {what}: partial {rf:.4f} dlogits_lr {rb:.4f}")
    if g == 1:       # the smoothness gradient alone: exact zeros
        only_tv = torch.zeros_like(coef)
        only_tv[:, 5] = coef[:, 5]
        assert bool((raw_bwd(lib, lrd, td, sd, only_tv.to(DEV), B, g, S, sr.TV) == 0).all())


def test_refused_calls_write_nothing(lib):
    B, g, S = 1, 3, 42
    lr, tgt, coef, _ = case_ref(sr.CASES[0], 0)
    lrd, td, cd = lr[:1].to(DEV).contiguous(), tgt[:1].to(DEV).contiguous(), coef[:1].to(DEV).contiguous()
    part, dl = Arena(6 * 8 * 4, 0xFF, DEV), Arena(9 * 4, 0xFF, DEV)
    sums = torch.ones(8, device=DEV)
    P = lambda t: t.data_ptr()
    for b, gg, s, terms, want in ((0, 3, 42, 7, BAD_SHAPE), (1, 0, 42, 7, BAD_SHAPE), (1, 3, 1, 7, BAD_SHAPE),
                                  (1, 4097, 42, 7, BAD_SHAPE), (1, 3, 2049, 7, BAD_SHAPE), (1, 3, 42, 8, UNSUPPORTED)):
        assert lib.sgl_op_seg_loss_ex_fwd(P(lrd), P(td), part.ptr, b, gg, s, terms, 0.25, stream()) == want
        assert lib.sgl_op_seg_loss_ex_bwd(P(lrd), P(td), P(sums), P(cd), dl.ptr, b, gg, s, terms, 0.25, 1e-6, 1e-6,
                                          stream()) == want
    assert lib.sgl_op_seg_loss_ex_fwd(P(lrd), None, part.ptr, B, g, S, 7, 0.25, stream()) == NULL
    assert lib.sgl_op_seg_loss_ex_bwd(P(lrd), P(td), None, P(cd), dl.ptr, B, g, S, 7, 0.25, 1e-6, 1e-6, stream()) == NULL
    torch.cuda.synchronize()
    assert part.untouched() and part.guards_intact() and dl.untouched() and dl.guards_intact()


# ---- combined_loss_from_lowres ----------------------------------------------------------------------------------
def compose(sums, w, S, wt, eps=1e-6, smooth=1e-6):
    """The wrapper's composition of the folded sums [B, 8] over the selection w [B] (float64, differentiable)."""
    n1 = w.sum().clamp(min=1.0)
    N, pairs = n1 * S * S, n1 * S * (S - 1)
    I, P, T = sums[:, 1], sums[:, 2], sums[:, 3]
    terms = [wt["bce_w"] * (sums[:, 0] * w).sum() / N, wt["focal_w"] * (sums[:, 4] * w).sum() / N,
             wt["dice_w"] * (1 - (2 * I / (P + T + eps) * w).sum() / n1),
             wt["boundary_w"] * (sums[:, 5] * w).sum() / N, wt["iou_w"] * (1 - (I / (P + T - I + smooth) * w).sum() / n1),
             wt["morph_w"] * ((sums[:, 6] + sums[:, 7]) * w).sum() / pairs]
    return sum(terms) * (w.sum() > 0), sum(t.abs() for t in terms)


def wrapper_ref(lib, lr, tgt, r, sel, wt, up):
    """Loss, its bound, d loss / d logits_lr and its bound for `up * combined_loss_from_lowres(...)`.
    Loss: the partial bounds folded (chunks more additions) and carried through the composition to first order, plus 32
    roundings of the composition's own fp32 arithmetic on the sum of its terms' magnitudes.
    Gradient: seg_loss_ex_bwd_ref on the very sums the kernel produced (the raw forward is bitwise reproducible) and the
    wrapper's coefficients; 8 more roundings for the coefficients' own fp32 arithmetic on the GPU."""
    B, g, S = lr.shape[0], lr.shape[-1], tgt.shape[-1]
    terms = (sr.FOCAL if wt["focal_w"] else 0) | (sr.BOUNDARY if wt["boundary_w"] else 0) | (sr.TV if wt["morph_w"] else 0)
    ref, bound = sr.seg_loss_ex_fwd_ref(lr, tgt, terms=terms, r=r)
    chunks = ref.shape[1]
    s64 = ref.sum(1).requires_grad_(True)
    sb = bound.sum(1) + chunks * EPS32 * ref.abs().sum(1)
    w = torch.tensor(sel, dtype=torch.float64)
    loss, mag = compose(s64, w, S, wt)
    (dsum,) = torch.autograd.grad(loss, s64, allow_unused=True)
    dsum = torch.zeros_like(s64) if dsum is None else dsum
    loss_bound = up * ((dsum.abs() * sb).sum() + 32 * EPS32 * mag.detach())
    part = raw_fwd(lib, lr.to(DEV), tgt.to(DEV), B, g, S, terms)
    sums = part.sum(1).cpu()                                   # the wrapper's own fold
    n1 = max(1.0, float(sum(sel)))
    N, pairs = n1 * S * S, n1 * S * (S - 1)
    row = torch.tensor([wt["bce_w"] / N, -wt["dice_w"] / n1, wt["focal_w"] / N, wt["boundary_w"] / N, -wt["iou_w"] / n1,
                        wt["morph_w"] / pairs], dtype=torch.float64) * up
    coef = (w[:, None] * row[None, :]).float()
    dref, dbound = sr.seg_loss_ex_bwd_ref(lr, tgt, sums, coef, terms=terms, r=r)
    dz, _ = sr.pixel_grad_ref(r, sums, coef, terms, 1e-6, 1e-6)
    dbound = dbound + 8 * EPS32 * (r["W"].t() @ dz.abs() @ r["W"])
    return up * loss.detach(), loss_bound, dref, dbound


SELECTIONS = {"all": lambda B: [True] * B, "alternating": lambda B: [b % 2 == 0 for b in range(B)],
              "none": lambda B: [False] * B}


@pytest.mark.parametrize("selection", list(SELECTIONS))
@pytest.mark.parametrize("case,mask_set", [(sr.CASES[0], 1), (sr.CASES[5], 1)], ids=str)
def test_wrapper_loss_and_gradient(pkg, lib, case, mask_set, selection):
    """Loss and logit_lr.grad under a non-unit upstream factor against the float64 composition; the empty selection gives
    exactly 0 with an exactly-zero gradient; two runs are bit-equal."""
    B, g, S = case
    lr, tgt, _, r = case_ref(case, mask_set)
    sel = SELECTIONS[selection](B)
    has = torch.tensor(sel, device=DEV)
    masks = tgt.to(DEV)[:, None]
    runs = []
    for _ in range(2):
        x = lr.to(DEV)[:, None].clone().requires_grad_(True)
        loss = 1.7 * pkg.heads.combined_loss_from_lowres(x, masks, has)
        loss.backward()
        runs.append((loss.detach().clone(), x.grad.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    loss, grad = runs[0]
    if selection == "none":
        assert loss.item() == 0.0 and bool((grad == 0).all())
        return
    want, lb, dref, dbound = wrapper_ref(lib, lr, tgt, r, sel, DEFAULTS, 1.7)
    print(f"LOSS {case} {selection}: got {loss.item():.9g} ref {want.item():.9g} bound {lb.item():.3g}")
    assert abs(loss.item() - want.item()) <= lb.item()
    rb = kr.assert_within(grad[:, 0].cpu(), dref, dbound, f"wrapper grad {case} {selection}")
    print(f"RATIO wrapper grad {case} {selection}: {rb:.4f}")
    for b in range(B):
        if not sel[b]:
            assert bool((grad[b] == 0).all())


def test_wrapper_bf16_logits_return_bf16_gradient(pkg, lib):
    case = sr.CASES[0]
    B, g, S = case
    lr, tgt, _, r = case_ref(case, 1, torch.bfloat16)          # the reference sees the bf16-rounded logits
    x = lr.to(DEV)[:, None].bfloat16().requires_grad_(True)
    loss = pkg.heads.combined_loss_from_lowres(x, tgt.to(DEV)[:, None])
    loss.backward()
    assert loss.dtype == torch.float32 and x.grad.dtype == torch.bfloat16
    want, lb, dref, dbound = wrapper_ref(lib, lr, tgt, r, [True] * B, DEFAULTS, 1.0)
    assert abs(loss.item() - want.item()) <= lb.item()
    kr.assert_within(x.grad[:, 0].float().cpu(), dref, dbound + kr.UNIT[torch.bfloat16] * dref.abs(), "bf16 grad")


def test_wrapper_with_bce_dice_weights_agrees_with_bce_dice_loss_from_lowres(pkg, lib):
    """Only bce_w and dice_w non-zero: terms = 0, and loss / gradient agree with the BCE/Dice path, each being within its
    own bound of the same float64 reference (kernel_ref.seg_loss_bwd_ref for the BCE/Dice kernels)."""
    case = sr.CASES[0]
    B, g, S = case
    lr, tgt, _, r = case_ref(case, 1)
    wt = dict(bce_w=0.7, focal_w=0.0, dice_w=0.35, boundary_w=0.0, iou_w=0.0, morph_w=0.0)
    assert pkg.head_ops.seg_terms_mask(wt["focal_w"], wt["boundary_w"], wt["morph_w"]) == 0
    masks = tgt.to(DEV)[:, None]
    a = lr.to(DEV)[:, None].clone().requires_grad_(True)
    b = lr.to(DEV)[:, None].clone().requires_grad_(True)
    la = pkg.heads.combined_loss_from_lowres(a, masks, **wt)
    lb_ = pkg.heads.bce_dice_loss_from_lowres(b, masks, bce_w=0.7, dice_w=0.35)
    la.backward()
    lb_.backward()
    want, lbound, dref, dbound = wrapper_ref(lib, lr, tgt, r, [True] * B, wt, 1.0)
    assert abs(la.item() - want.item()) <= lbound.item() and abs(lb_.item() - want.item()) <= lbound.item()
    kr.assert_within(a.grad[:, 0].cpu(), dref, dbound, "enhanced path, bce/dice weights")
    kr.assert_within(b.grad[:, 0].cpu(), dref, dbound, "bce/dice path")


# ---- the model ---------------------------------------------------------------------------------------------------
# name -> (weights, loss tolerance, gradient tolerance).  test_training_loss_equals_forward_then_mtl_loss holds the same
# comparison with two of the six terms to 2e-6 / 5e-5, and no term needs more: observed on the MI355X, loss relative error 0
# for both sets of weights, worst parameter-gradient error 4.6e-7 (iou_focused) and 3.5e-7 (defaults).
MODEL_CASES = {"iou_focused": (IOU_FOCUSED, 2e-6, 5e-5), "defaults": (DEFAULTS, 2e-6, 5e-5)}


@pytest.mark.parametrize("name", list(MODEL_CASES))
def test_training_loss_enhanced_equals_forward_then_combined_loss(pkg, lib, name):
    """SigLIP2MTL.training_loss(enhanced=True) against forward() + CE + lam * combined_segmentation_loss on the images with
    a mask (mtl_loss(enhanced=True) with the given weights; for `defaults` mtl_loss itself), values and gradients, on the
    `hostile` config in fp32 mode, exactly-zero gradients excluded as in test_training_loss_equals_forward_then_mtl_loss.
    Then the default call: bit for bit CE + lam * bce_dice_loss_from_lowres composed by hand."""
    wt, loss_tol, grad_tol = MODEL_CASES[name]
    H = pkg.heads
    cfg = pkg.get_config("hostile")
    enc = pkg.SiglipVisionModelHIP(cfg, compute_dtype="fp32")
    enc.load_state_dict(pkg.weights.seeded_state_dict(cfg, seed=13))
    torch.manual_seed(0)
    model = H.SigLIP2MTL(enc, seg_layers=(0, 1, -1), embed_dim=32, freeze_below=1).cuda()
    x = pkg.weights.seeded_pixels(3, 56, 56, seed=17).cuda()
    y = torch.tensor([2, 0, 1]).cuda()
    masks = (pkg.weights.seeded_tensor("masks", (3, 1, 56, 56), 1.0) > 0.2).float().cuda()
    has = torch.tensor([True, False, True]).cuda()
    cls, seg = model(x)
    if name == "defaults":
        ref = H.mtl_loss(cls, seg, y, masks, has, lam_seg=0.8, enhanced=True)
    else:
        ref = F.cross_entropy(cls, y) + 0.8 * H.combined_segmentation_loss(seg[has], masks[has], **wt)
    ref.backward()
    want = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    model.zero_grad(set_to_none=True)
    loss, cls2, seg_lr = model.training_loss(x, y, masks, has, lam_seg=0.8, enhanced=True, **wt)
    loss.backward()
    assert seg_lr.shape == (3, 1, 4, 4) and torch.equal(cls, cls2)
    lerr = abs(loss.item() - ref.item()) / abs(ref.item())
    worst = 0.0
    for n, p in model.named_parameters():
        if n in want and not (n.endswith("k_proj.bias") or n.endswith("in_proj_bias")):   # exactly-zero gradients: noise
            err = (p.grad - want[n]).abs().max().item() / (want[n].abs().max().item() + 1e-30)
            worst = max(worst, err)
            assert err < grad_tol, (n, err)
    print(f"MODEL {name}: loss rel err {lerr:.3g} worst grad err {worst:.3g}")
    assert lerr <= loss_tol, lerr
    # the default call is the BCE/Dice path, unchanged
    model.zero_grad(set_to_none=True)
    loss_d, _, lr_d = model.training_loss(x, y, masks, has, lam_seg=0.8)
    cls_h, lr_h = model(x, return_lowres=True)
    loss_h = F.cross_entropy(cls_h.float(), y) + 0.8 * H.bce_dice_loss_from_lowres(lr_h, masks, has, bce_w=1.0, dice_w=0.5)
    assert torch.equal(loss_d, loss_h) and torch.equal(lr_d, lr_h)
    (gd,) = torch.autograd.grad(loss_d, lr_d)
    (gh,) = torch.autograd.grad(loss_h, lr_h)
    assert torch.equal(gd, gh)
