"""The HIP-backed operations of the heads: autograd Functions over the ``sgl_op_*`` kernels and, for each, ONE dispatcher that
holds the rule for when the kernel is eligible and the torch composition used when it is not: ``linear_tokens``,
``depthwise3x3``, ``gate_mul``, ``bce_dice_loss_from_lowres``, ``combined_loss_from_lowres``, ``seg_eval_from_lowres``,
``l2norm_temporal_mean``.  Every launch goes through
``lib.call`` (guard and stream of the device the operands live on).  ``heads.py`` holds the modules and losses built on these.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch.utils.weak import WeakIdKeyDictionary

from . import lib as _lib

_BF16 = _lib.SGL_DTYPE_BF16


class WeightCache:
    """bf16 GEMM operands of the decoder's weights: the decoder has ~40 Linear layers and used to re-cast and re-transpose
    each one on every call.  One entry per live parameter, keyed on the parameter OBJECT (never on its address: the caching
    allocator hands a freed parameter's address to the next model's weights); an entry dies with its parameter and is
    re-made when the parameter changed (optimizer steps bump ``_version``; ``.data`` swaps move ``data_ptr``)."""

    def __init__(self):
        self._entries = WeakIdKeyDictionary()      # parameter -> [(version, data_ptr), bf16 W, bf16 Wᵀ or None]

    def __len__(self):
        return len(self._entries)

    def get(self, weight: torch.Tensor, want_t: bool = False):
        """(W, Wᵀ or None) of a (N, K) Linear or (N, K, 1, 1) convolution weight: W is the contiguous bf16 [Np, K] matrix,
        Np = round_up(N, 8) (the GEMM's column granularity) with rows N.. zero; Wᵀ [K, Np] is made on the first
        ``want_t`` and kept."""
        key = (weight._version, weight.data_ptr())
        entry = self._entries.get(weight)
        if entry is None or entry[0] != key:
            w = weight.detach().flatten(1).to(torch.bfloat16)
            if w.shape[0] % 8:
                w = F.pad(w, (0, 0, 0, 8 - w.shape[0] % 8))
            entry = self._entries[weight] = [key, w.contiguous(), None]
        if want_t and entry[2] is None:
            entry[2] = entry[1].t().contiguous()
        return entry[1], entry[2]

    def drop(self, weight: torch.Tensor) -> bool:
        """Forget ``weight``'s entry (the next ``get`` re-casts it); says whether there was one."""
        return self._entries.pop(weight, None) is not None


_weights = WeightCache()


def invalidate_weights(module: torch.nn.Module) -> int:
    """Drop the cached bf16 operands of every parameter of ``module`` (and its sub-modules): the decoder's counterpart of
    ``WeightShadows.invalidate``.  Needed only after a write the key cannot see, which is an in-place write through
    ``p.data`` (``p.data.copy_(...)``: ``p.data`` has a version counter of its own, so ``p._version`` and ``data_ptr``
    both stay).  Returns the number of entries dropped.  A forward whose backward has not run yet keeps the operands it
    used."""
    return sum(_weights.drop(p) for p in module.parameters())
_scratch: dict = {}       # device -> 64 MiB split-K scratch, reused by every call (stream-ordered)


def _split_scratch(dev):
    buf = _scratch.get(dev)
    if buf is None:
        buf = _scratch[dev] = torch.empty(64 << 20, device=dev, dtype=torch.uint8)
    return buf


def _pad_last(t: torch.Tensor, n: int) -> torch.Tensor:
    """`t` with its last dimension zero-padded to `n` entries."""
    return t if t.shape[-1] == n else F.pad(t, (0, n - t.shape[-1]))


def _aligned16(t: torch.Tensor) -> torch.Tensor:
    """`t` itself when its storage pointer is 16-byte aligned, otherwise a fresh copy (`.contiguous()` does not move a
    contiguous offset view such as `buf[1:]`; the vector kernels need 16-byte aligned operands)."""
    return t if t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.contiguous_format)


# ---------------------------------------------------------------------------------------------------------
# Linear / 1x1 convolution
# ---------------------------------------------------------------------------------------------------------
class _HipLinearFn(torch.autograd.Function):
    """y = x Wᵀ + b on bf16 token-major activations through the encoder's own MFMA GEMM kernels (sgl_op_gemm_nt /
    sgl_op_gemm_tn): the decoder's tall-skinny shapes (46656 x 512 x 1152, 46656 x 512 x 512 ...) are where the
    library GEMM picks 110-240 TFLOP/s kernels.  Used under autocast only (bf16 operands, fp32 accumulate: the
    arithmetic autocast's F.linear does); fp32 callers keep F.linear.  `weight` is the parameter itself, (N, K) or
    (N, K, 1, 1); the GEMMs run at Np = round_up(N, 8) columns on zero-padded operands (the 1-channel mask head)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        M, K = x.shape
        N = weight.shape[0]
        xb = x.to(torch.bfloat16).contiguous()
        wb, _ = _weights.get(weight)
        Np = wb.shape[0]
        bf = None if bias is None else _pad_last(bias.detach().float(), Np).contiguous()
        y = torch.empty(M, Np, device=x.device, dtype=torch.bfloat16)
        _lib.call("sgl_op_gemm_nt", x.device, _BF16, xb.data_ptr(), K, wb.data_ptr(), K, M, Np, K, _lib.EPI_STORE,
                  y.data_ptr(), Np, None, 0, _lib.ptr(bf), None, 0, None, 0, None, 1, 1, 1, 8, 8, 1)
        ctx.save_for_backward(xb, wb)
        ctx.weight = weight
        ctx.has_bias = bias is not None
        ctx.xdtype = x.dtype
        return y if Np == N else y[:, :N]

    @staticmethod
    def backward(ctx, dy):
        xb, wb = ctx.saved_tensors
        M, K = xb.shape
        N, Np = ctx.weight.shape[0], wb.shape[0]
        dev = xb.device
        dyb = _pad_last(dy.to(torch.bfloat16), Np).contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:   # dX[M,K] = dY[M,Np] · W[Np,K]: NT form with the K x Np transpose of W as "B"
            cur, cur_t = _weights.get(ctx.weight, want_t=True)
            wt = cur_t if cur is wb else wb.t().contiguous()      # the cached pair only if it is still this forward's weight
            dx = torch.empty(M, K, device=dev, dtype=torch.bfloat16)
            _lib.call("sgl_op_gemm_nt", dev, _BF16, dyb.data_ptr(), Np, wt.data_ptr(), Np, M, K, Np, _lib.EPI_STORE,
                      dx.data_ptr(), K, None, 0, None, None, 0, None, 0, None, 1, 1, 1, 8, 8, 1)
            dx = dx.to(ctx.xdtype)
        if ctx.needs_input_grad[1]:   # dW[Np,K] = dYᵀ · X
            dw = torch.empty(Np, K, device=dev, dtype=torch.float32)
            scratch = _split_scratch(dev)   # split-K slabs: deterministic sum
            _lib.call("sgl_op_gemm_tn_ws", dev, _BF16, dyb.data_ptr(), Np, xb.data_ptr(), K, M, Np, K, 0, dw.data_ptr(), K,
                      0, scratch.data_ptr(), scratch.numel())
            dw = dw[:N].to(ctx.weight.dtype).view(ctx.weight.shape)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = (dyb.float().sum(0) if M < 64 else _hip_colsum(dyb, M, Np))[:N]
        return dx, dw, db


def _hip_colsum(t, M, N):
    out = torch.empty(N, device=t.device, dtype=torch.float32)
    nbytes = ((M + 511) // 512 if (M + 511) // 512 < 256 else 256) * N * 4
    scratch = torch.empty(max(nbytes, 4), device=t.device, dtype=torch.uint8)
    _lib.call("sgl_op_colsum", t.device, _BF16, t.data_ptr(), N, M, N, out.data_ptr(), 0, scratch.data_ptr(),
              scratch.numel())
    return out


@torch.compiler.disable
def _hip_linear(x2d, weight, bias):
    return _HipLinearFn.apply(x2d, weight, bias)


def linear_tokens(x: torch.Tensor, weight: torch.Tensor, bias) -> torch.Tensor:
    """F.linear on (..., K) token-major data with a Linear's (N, K) or a 1x1 convolution's (N, K, 1, 1) weight.  Under CUDA
    bf16 autocast, when K % 8 == 0 and there are at least 64 rows, it runs on the HIP GEMMs (bf16 operands, fp32
    accumulate: the arithmetic autocast's F.linear does; 256x256-tile kernels for large shapes, 128x128-tile ones for
    narrow ones).  fp32 callers (strict parity runs, CPU) keep F.linear."""
    K, N = x.shape[-1], weight.shape[0]
    if (x.is_cuda and torch.is_autocast_enabled() and torch.get_autocast_dtype("cuda") == torch.bfloat16
            and K % 8 == 0 and x.numel() // K >= 64):
        return _hip_linear(x.reshape(-1, K), weight, bias).reshape(*x.shape[:-1], N)
    return F.linear(x, weight.flatten(1), bias)


# ---------------------------------------------------------------------------------------------------------
# depthwise 3x3
# ---------------------------------------------------------------------------------------------------------
class _DepthwiseConv3x3Fn(torch.autograd.Function):
    """Depthwise 3x3 (padding 1) on channels-last (B, gh, gw, E) CUDA tensors through the HIP kernels of
    csrc/decoder.hip: forward, data gradient (same stencil, flipped taps) and the two-stage weight/bias gradient."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        if x.dtype not in (torch.float32, torch.bfloat16):
            x = x.float()
        x = _aligned16(x.contiguous())
        B, gh, gw, E = x.shape
        w = weight.detach().float().reshape(E, 9).t().contiguous()      # tap-major [9][E] (see siglip_hip.h)
        b = None if bias is None else _aligned16(bias.detach().float().contiguous())
        y = torch.empty_like(x)
        _lib.call("sgl_op_dwconv3x3", x.device, x.data_ptr(), _lib.dtype_code(x.dtype), w.data_ptr(), _lib.ptr(b),
                  y.data_ptr(), B, gh, gw, E, 0)
        ctx.save_for_backward(x, w)
        ctx.has_bias = bias is not None
        ctx.wdtype = weight.dtype
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = _aligned16(dy.to(x.dtype).contiguous())
        B, gh, gw, E = x.shape
        dt = _lib.dtype_code(x.dtype)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            _lib.call("sgl_op_dwconv3x3", x.device, dy.data_ptr(), dt, w.data_ptr(), None, dx.data_ptr(), B, gh, gw, E, 1)
        dw = db = None
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            dw10 = torch.empty(10, E, device=x.device, dtype=torch.float32)   # nine tap rows + the bias row
            nbytes = _lib.load().sgl_op_dwconv3x3_wgrad_scratch_bytes(B, gh, gw, E)
            scratch = torch.empty(nbytes, device=x.device, dtype=torch.uint8)
            _lib.call("sgl_op_dwconv3x3_wgrad", x.device, x.data_ptr(), dy.data_ptr(), dt, dw10.data_ptr(), 0,
                      scratch.data_ptr(), nbytes, B, gh, gw, E)
            dw = dw10[:9].t().reshape(E, 1, 3, 3).to(ctx.wdtype)
            db = dw10[9] if ctx.has_bias else None
        return dx, dw, db


@torch.compiler.disable
def _hip_dwconv(x, weight, bias):
    return _DepthwiseConv3x3Fn.apply(x, weight, bias)


def depthwise3x3(x: torch.Tensor, weight: torch.Tensor, bias) -> torch.Tensor:
    """Depthwise 3x3, zero padding 1, on channels-last data (B, gh, gw, E) with an nn.Conv2d(E, E, 3, padding=1, groups=E)
    weight (E, 1, 3, 3): one HBM pass (csrc/decoder.hip) on CUDA tensors whose E the kernel's vector layout divides,
    otherwise nine shifted multiply-adds (the same arithmetic; MIOpen has only a naive fp32 NHWC solver for it)."""
    e = x.shape[-1]
    if x.is_cuda and e % 8 == 0 and e <= 1024 and 256 % (e // 8) == 0 and 256 % (e // 4) == 0:
        return _hip_dwconv(x, weight, bias)
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))    # pad gw and gh by one
    gh, gw = x.shape[1], x.shape[2]
    out = None
    for dy in range(3):
        for dx in range(3):
            term = xp[:, dy:dy + gh, dx:dx + gw, :] * weight[:, 0, dy, dx]
            out = term if out is None else out + term
    return out + bias if bias is not None else out


# ---------------------------------------------------------------------------------------------------------
# decoder tail: gate, loss from the low-res logits
# ---------------------------------------------------------------------------------------------------------
def _gate_dtype(g: torch.Tensor) -> torch.dtype:
    return g.dtype if g.dtype in (torch.float32, torch.bfloat16) else torch.float32


class _GateMulFn(torch.autograd.Function):
    """y = sigmoid(g) * x in one HBM pass (csrc/decoder_tail.hip), backward (dg w.r.t. the PRE-sigmoid gate, dx) in one
    more: the SE-style gate of the SID decoder (`gate * x`, Siglip2sidafrozen.py:741-742) on (B*N, E*K) activations."""

    @staticmethod
    def forward(ctx, g, x):
        dt = _gate_dtype(g)
        g2, x2 = g.to(dt).contiguous(), x.to(dt).contiguous()
        y = torch.empty_like(x2)
        _lib.call("sgl_op_gate_mul", g2.device, g2.data_ptr(), x2.data_ptr(), y.data_ptr(), g2.numel(), _lib.dtype_code(dt))
        ctx.save_for_backward(g2, x2)
        ctx.gdt, ctx.xdt = g.dtype, x.dtype
        return y

    @staticmethod
    def backward(ctx, dy):
        g2, x2 = ctx.saved_tensors
        dy2 = _aligned16(dy.to(g2.dtype).contiguous())
        dg = torch.empty_like(g2) if ctx.needs_input_grad[0] else None
        dx = torch.empty_like(x2) if ctx.needs_input_grad[1] else None
        _lib.call("sgl_op_gate_mul_bwd", g2.device, dy2.data_ptr(), g2.data_ptr(), x2.data_ptr(), _lib.ptr(dg), _lib.ptr(dx),
                  g2.numel(), _lib.dtype_code(g2.dtype))
        return (None if dg is None else dg.to(ctx.gdt)), (None if dx is None else dx.to(ctx.xdt))


@torch.compiler.disable
def gate_mul(gate_pre: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """sigmoid(gate_pre) * x: the HIP kernel on CUDA tensors of one shape with at least 4096 elements, a whole number of
    16-byte vectors and aligned storage, torch's composition otherwise."""
    nv = 8 if gate_pre.dtype == torch.bfloat16 else 4
    if gate_pre.is_cuda and gate_pre.shape == x.shape and gate_pre.numel() % nv == 0 and gate_pre.numel() >= 4096:
        # a contiguous offset view (buf[1:]) keeps its misaligned pointer through .to(dt).contiguous() when it already has
        # the kernel's dtype (another dtype is cast into a fresh buffer): sgl_op_gate_mul refuses such a pointer
        dt = _gate_dtype(gate_pre)
        misaligned = any(t.dtype == dt and t.is_contiguous() and t.data_ptr() % 16 for t in (gate_pre, x))
        if not misaligned:
            return _GateMulFn.apply(gate_pre, x)
    return torch.sigmoid(gate_pre) * x


class _SegLossFromLowresFn(torch.autograd.Function):
    """`bce_dice_loss(F.interpolate(logit_lr, (S,S), 'bilinear'), masks)` over the images flagged in `sel`, without
    ever forming the (B,1,S,S) logits: csrc/decoder_tail.hip evaluates every output pixel from its four low-res logits in
    registers (forward: per-image partial sums; backward: transposed interpolation gathered per low-res pixel, fixed order).
    No host synchronisation: an empty selection gives 0 (the reference skips the term, Siglip2sidafrozen.py:1380-1389)."""

    @staticmethod
    def forward(ctx, logit_lr, masks, sel, bce_w, dice_w, eps):
        B, g = logit_lr.shape[0], logit_lr.shape[-1]
        S = masks.shape[-1]
        lr = logit_lr.detach().reshape(B, g, g).float().contiguous()
        t = masks.reshape(B, S, S).float().contiguous()
        chunks = _lib.load().sgl_op_seg_loss_chunks(S)
        partial = torch.empty(B, chunks, 4, device=lr.device, dtype=torch.float32)
        _lib.call("sgl_op_seg_loss_fwd", lr.device, lr.data_ptr(), t.data_ptr(), partial.data_ptr(), B, g, S)
        sums = partial.sum(1)                                   # (B, 4), fixed order
        w = sel.to(torch.float32)
        n = w.sum()
        nz = (n > 0).to(torch.float32)
        n1 = n.clamp(min=1.0)
        bce = (sums[:, 0] * w).sum() / (n1 * float(S * S))
        dice_b = 2.0 * sums[:, 1] / (sums[:, 2] + sums[:, 3] + eps)
        dice = 1.0 - (dice_b * w).sum() / n1
        loss = (bce_w * bce + dice_w * dice) * nz
        ctx.save_for_backward(lr, t, sums, w, n1, nz)
        ctx.cfg = (B, g, S, bce_w, dice_w, eps, logit_lr.shape, logit_lr.dtype)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        lr, t, sums, w, n1, nz = ctx.saved_tensors
        B, g, S, bce_w, dice_w, eps, shape, dtype = ctx.cfg
        up = dloss.float() * nz
        coef = torch.stack([up * bce_w * w / (n1 * float(S * S)), -up * dice_w * w / n1], dim=1).contiguous()
        dlr = torch.empty_like(lr)
        _lib.call("sgl_op_seg_loss_bwd", lr.device, lr.data_ptr(), t.data_ptr(), sums.contiguous().data_ptr(),
                  coef.data_ptr(), dlr.data_ptr(), B, g, S, float(eps))
        return dlr.reshape(shape).to(dtype), None, None, None, None, None


@torch.compiler.disable
def bce_dice_loss_from_lowres(logit_lr: torch.Tensor, masks: torch.Tensor, has_mask: torch.Tensor = None,
                              bce_w: float = 1.0, dice_w: float = 0.5, eps: float = 1e-6) -> torch.Tensor:
    """`bce_dice_loss(upsample(logit_lr)[has_mask], masks[has_mask])` (Siglip2sidafrozen.py:174-181,743) from the (B,1,g,g)
    logits of `SegFormerMaskDecoder(..., return_lowres=True)`; CUDA only (HIP kernels), fp32 statistics."""
    if not logit_lr.is_cuda:
        raise RuntimeError("bce_dice_loss_from_lowres runs on the GPU (HIP kernels); use bce_dice_loss on CPU tensors")
    if has_mask is None:
        has_mask = torch.ones(logit_lr.shape[0], dtype=torch.bool, device=logit_lr.device)
    return _SegLossFromLowresFn.apply(logit_lr, masks, has_mask, float(bce_w), float(dice_w), float(eps))


_FOCAL_ALPHA = 0.25       # focal_loss's alpha at the reference's call site (Siglip2sidafrozen.py:155; gamma = 2 is the kernel's)


def seg_terms_mask(focal_w: float, boundary_w: float, morph_w: float) -> int:
    """The `terms` bits of sgl_op_seg_loss_ex_*: an optional per-pixel term is computed only when its weight is non-zero."""
    return ((_lib.SEG_TERM_FOCAL if focal_w != 0 else 0) | (_lib.SEG_TERM_BOUNDARY if boundary_w != 0 else 0)
            | (_lib.SEG_TERM_TV if morph_w != 0 else 0))


class _CombinedLossFromLowresFn(torch.autograd.Function):
    """`combined_segmentation_loss(F.interpolate(logit_lr, (S,S), 'bilinear'), masks)` over the images flagged in `sel`, the
    enhanced counterpart of `_SegLossFromLowresFn` (same operands, same fold, no host synchronisation, an empty selection
    gives 0): sgl_op_seg_loss_ex_fwd / _bwd."""

    @staticmethod
    def forward(ctx, logit_lr, masks, sel, weights, eps, smooth):
        bce_w, focal_w, dice_w, boundary_w, iou_w, morph_w = weights
        B, g = logit_lr.shape[0], logit_lr.shape[-1]
        S = masks.shape[-1]
        terms = seg_terms_mask(focal_w, boundary_w, morph_w)
        lr = logit_lr.detach().reshape(B, g, g).float().contiguous()
        t = masks.reshape(B, S, S).float().contiguous()
        chunks = _lib.load().sgl_op_seg_loss_chunks(S)
        partial = torch.empty(B, chunks, 8, device=lr.device, dtype=torch.float32)
        _lib.call("sgl_op_seg_loss_ex_fwd", lr.device, lr.data_ptr(), t.data_ptr(), partial.data_ptr(), B, g, S, terms,
                  _FOCAL_ALPHA)
        sums = partial.sum(1)                                   # (B, 8), fixed order
        w = sel.to(torch.float32)
        n = w.sum()
        nz = (n > 0).to(torch.float32)
        n1 = n.clamp(min=1.0)
        npix, npairs = n1 * float(S * S), n1 * float(S * (S - 1))
        inter, psum, tsum = sums[:, 1], sums[:, 2], sums[:, 3]
        bce = (sums[:, 0] * w).sum() / npix
        focal = (sums[:, 4] * w).sum() / npix
        boundary = (sums[:, 5] * w).sum() / npix
        dice = 1.0 - (2.0 * inter / (psum + tsum + eps) * w).sum() / n1
        iou = 1.0 - (inter / (psum + tsum - inter + smooth) * w).sum() / n1
        morph = ((sums[:, 6] + sums[:, 7]) * w).sum() / npairs
        loss = (bce_w * bce + focal_w * focal + dice_w * dice + boundary_w * boundary + iou_w * iou + morph_w * morph) * nz
        ctx.save_for_backward(lr, t, sums, w, n1, nz)
        ctx.cfg = (B, g, S, terms, weights, eps, smooth, logit_lr.shape, logit_lr.dtype)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        lr, t, sums, w, n1, nz = ctx.saved_tensors
        B, g, S, terms, (bce_w, focal_w, dice_w, boundary_w, iou_w, morph_w), eps, smooth, shape, dtype = ctx.cfg
        up = dloss.float() * nz
        per_px, per_img, per_pair = up * w / (n1 * float(S * S)), up * w / n1, up * w / (n1 * float(S * (S - 1)))
        coef = torch.stack([bce_w * per_px, -dice_w * per_img, focal_w * per_px, boundary_w * per_px, -iou_w * per_img,
                            morph_w * per_pair], dim=1).contiguous()
        dlr = torch.empty_like(lr)
        _lib.call("sgl_op_seg_loss_ex_bwd", lr.device, lr.data_ptr(), t.data_ptr(), sums.contiguous().data_ptr(),
                  coef.data_ptr(), dlr.data_ptr(), B, g, S, terms, _FOCAL_ALPHA, float(eps), float(smooth))
        return dlr.reshape(shape).to(dtype), None, None, None, None, None


@torch.compiler.disable
def combined_loss_from_lowres(logit_lr: torch.Tensor, masks: torch.Tensor, has_mask: torch.Tensor = None,
                              bce_w: float = 0.4, focal_w: float = 0.3, dice_w: float = 0.5, boundary_w: float = 0.4,
                              iou_w: float = 0.4, morph_w: float = 0.2, eps: float = 1e-6,
                              smooth: float = 1e-6) -> torch.Tensor:
    """`combined_segmentation_loss(upsample(logit_lr)[has_mask], masks[has_mask])` (Siglip2sidafrozen.py:142-172, the
    `--use_enhanced_loss` branch of the train step) from the (B,1,g,g) logits of `SegFormerMaskDecoder(...,
    return_lowres=True)`; CUDA only (HIP kernels), fp32 statistics, the (B,1,S,S) logits are never formed.  A term whose
    weight is zero is not computed.  `smooth` is `iou_loss`'s."""
    if not logit_lr.is_cuda:
        raise RuntimeError("combined_loss_from_lowres runs on the GPU (HIP kernels); use combined_segmentation_loss on CPU "
                           "tensors")
    if has_mask is None:
        has_mask = torch.ones(logit_lr.shape[0], dtype=torch.bool, device=logit_lr.device)
    weights = tuple(float(v) for v in (bce_w, focal_w, dice_w, boundary_w, iou_w, morph_w))
    return _CombinedLossFromLowresFn.apply(logit_lr, masks, has_mask, weights, float(eps), float(smooth))


def check_cuts(cuts) -> None:
    """The contract `sgl_op_seg_eval` leaves to its caller: 1..64 finite-or-infinite (never NaN), strictly increasing cuts."""
    c = [float(v) for v in cuts]
    if not 1 <= len(c) <= 64:
        raise ValueError(f"seg_eval takes 1 to 64 cuts, not {len(c)}")
    if any(v != v for v in c) or any(b <= a for a, b in zip(c, c[1:])):
        raise ValueError("seg_eval cuts must be strictly increasing")


@torch.no_grad()
@torch.compiler.disable
def seg_eval_from_lowres(logit_lr: torch.Tensor, masks: torch.Tensor, has_mask: torch.Tensor = None, cuts=None,
                         auc_hist: torch.Tensor = None) -> torch.Tensor:
    """Per-image pixel counts between consecutive logit cuts, straight from the (B,1,g,g) logits of
    `SegFormerMaskDecoder(..., return_lowres=True)`: `hist[b, c, k]` (int32, (B, 2, K+1)) is the number of pixels of class
    c (1 where `masks` > 0.5) of image b whose bilinearly up-sampled logit z has exactly k of the K cuts strictly below it,
    so `z > cuts[j]` holds for the pixels with k > j.  One HIP launch (csrc/decoder_tail.hip: seg_eval), no host
    synchronisation, the (B,1,S,S) logits are never formed.  CUDA only.

    logit_lr   fp32 / bf16 / fp16, upcast to fp32 as `bce_dice_loss_from_lowres` does (the same fp32 z).
    masks      (B,1,S,S) or (B,S,S); float (any float dtype, read as fp32), uint8 or bool (read as bytes).
    has_mask   (B,) selection; images outside it get an all-zero row (None: every image).
    cuts       strictly increasing logit values, K <= 64: a sequence or CPU tensor is checked and uploaded; a CUDA fp32
               tensor is used as it is (checking it would need a synchronisation: the order is then the caller's contract).
    auc_hist   optional (2, 4096) int64 CUDA tensor that the launch ADDS to: per class, pixels per logit bin of width 1/128
               on [-16, 16) (`lib.SEG_EVAL_AUC_BINS` bins; outside values in the end bins, NaN in bin 0)."""
    if not logit_lr.is_cuda or not masks.is_cuda:
        raise RuntimeError("seg_eval_from_lowres runs on the GPU (HIP kernels); MaskMetrics.update_from_hist takes counts "
                           "made elsewhere")
    if cuts is None:
        raise ValueError("seg_eval_from_lowres needs the logit cuts")
    dev = logit_lr.device
    B, g = logit_lr.shape[0], logit_lr.shape[-1]
    S = masks.shape[-1]
    if logit_lr.numel() != B * g * g or masks.numel() != B * S * S:
        raise ValueError(f"expected (B,1,g,g) logits and (B,1,S,S) masks, got {tuple(logit_lr.shape)} and {tuple(masks.shape)}")
    lr = logit_lr.detach().reshape(B, g, g).float().contiguous()
    if masks.dtype == torch.bool:
        t, tcode = masks.contiguous().view(torch.uint8), _lib.SGL_DTYPE_U8
    elif masks.dtype == torch.uint8:
        t, tcode = masks.contiguous(), _lib.SGL_DTYPE_U8
    elif masks.dtype.is_floating_point:
        t, tcode = masks.float().contiguous(), _lib.SGL_DTYPE_F32
    else:
        raise ValueError(f"masks must be float, uint8 or bool, not {masks.dtype}")
    if isinstance(cuts, torch.Tensor) and cuts.is_cuda:
        if cuts.dtype != torch.float32 or cuts.dim() != 1 or not 1 <= cuts.numel() <= 64 or cuts.device != dev:
            raise ValueError("device cuts must be a 1-D fp32 tensor of 1 to 64 values on the logits' device")
        c = cuts.contiguous()
    else:
        vals = cuts.tolist() if isinstance(cuts, torch.Tensor) else list(cuts)
        check_cuts(vals)
        c = torch.tensor(vals, dtype=torch.float32).to(dev)
    K = c.numel()
    sel = None if has_mask is None else has_mask.to(device=dev, dtype=torch.uint8).contiguous()
    if sel is not None and sel.numel() != B:
        raise ValueError(f"has_mask must have {B} entries")
    if auc_hist is not None and (auc_hist.dtype != torch.int64 or tuple(auc_hist.shape) != (2, _lib.SEG_EVAL_AUC_BINS)
                                 or not auc_hist.is_contiguous() or auc_hist.device != dev):
        raise ValueError(f"auc_hist must be a contiguous (2, {_lib.SEG_EVAL_AUC_BINS}) int64 tensor on the logits' device")
    hist = torch.empty(B, 2, K + 1, device=dev, dtype=torch.int32)
    _lib.call("sgl_op_seg_eval", dev, lr.data_ptr(), t.data_ptr(), tcode, _lib.ptr(sel), c.data_ptr(), K, hist.data_ptr(),
              _lib.ptr(auc_hist), B, g, S)
    return hist


# ---------------------------------------------------------------------------------------------------------
# video head: per-frame L2-norm, temporal mean
# ---------------------------------------------------------------------------------------------------------
class _L2NormTemporalMeanFn(torch.autograd.Function):
    """(B*T, D) frame embeddings -> per-frame L2-norm -> mean over the T frames of a clip -> (B, D), one HIP launch forward
    and one backward (csrc/video_tail.hip) instead of norm / div / view / mean and their four backward kernels
    (hidf_video_classifier.py:308-316)."""

    @staticmethod
    def forward(ctx, f, batch_size):
        f32 = f.float().contiguous()
        BT, D = f32.shape
        T = BT // batch_size
        out = torch.empty(batch_size, D, device=f.device, dtype=torch.float32)
        inv = torch.empty(BT, device=f.device, dtype=torch.float32)
        _lib.call("sgl_op_l2norm_tmean_fwd", f.device, f32.data_ptr(), out.data_ptr(), inv.data_ptr(), batch_size, T, D)
        ctx.save_for_backward(f32, inv)
        ctx.dims, ctx.dtype = (batch_size, T, D), f.dtype
        return out.to(f.dtype)

    @staticmethod
    def backward(ctx, dout):
        f32, inv = ctx.saved_tensors
        B, T, D = ctx.dims
        g = dout.float().contiguous()
        df = torch.empty_like(f32)
        _lib.call("sgl_op_l2norm_tmean_bwd", f32.device, f32.data_ptr(), inv.data_ptr(), g.data_ptr(), df.data_ptr(), B, T, D)
        return df.to(ctx.dtype), None


@torch.compiler.disable
def l2norm_temporal_mean(frame_features: torch.Tensor, batch_size: int) -> torch.Tensor:
    """`(f / f.norm(dim=-1, keepdim=True)).view(B, T, D).mean(1)`; fused HIP kernels on CUDA (B*T, D) tensors, PyTorch ops
    elsewhere."""
    if frame_features.is_cuda and frame_features.dim() == 2 and frame_features.shape[0] % batch_size == 0:
        return _L2NormTemporalMeanFn.apply(frame_features, batch_size)
    f = frame_features / frame_features.norm(dim=-1, keepdim=True)
    return f.view(batch_size, -1, frame_features.shape[-1]).mean(dim=1)
