"""GPU input pipeline (first slice): the reference's per-batch GPU transform

    gpu_transform = nn.Sequential(K.Resize(target_resolution, antialias=True),
                                  K.Normalize(mean=[0.5]*3, std=[0.5]*3))            cifake_binary_classifier.py:1791-1794
    images = gpu_transform(images);  [MixUp: lam*images + (1-lam)*images[index]]      cifake_binary_classifier.py:808-817

as ONE HIP kernel (``csrc/preprocess.hip``) that can also write its result directly in the layout the patch-embedding GEMM
reads (``to_patch_operand``), so that the fp32 (B,3,S,S) pixel tensor and the encoder's im2col pass both disappear:

    enc(patches=to_patch_operand(uint8_nhwc_batch, enc.config))      instead of      enc(pixel_values=gpu_transform(x))

Sources: decoded ``uint8`` images in NHWC (B,H,W,3) — what a JPEG decoder hands over — or ``float32`` NCHW in [0,1] (what the
reference's CPU transform ``Resize + ToTensor`` produces).  Resampling is torch's antialiased bilinear filter
(``F.interpolate(mode="bilinear", antialias=True)``, the arithmetic torchvision ``Resize(antialias=True)`` runs in the
reference's CPU transform, cifake…:1795-1797); kornia itself is not installed here, so equality with ``K.Resize`` is
"parity unpinned".  CUDA only: there is no CPU path.

Training side (hidf_video_classifier.py ``--data_augmentation``): ``augment_resize_normalize`` / ``GpuTransform(...,
data_augmentation=True)`` insert flip, rotation and colour jitter between resize and normalise; with ``differentiable=True``
they are differentiable with respect to a float source (one ``sgl_op_preprocess_aug_bwd``, which recomputes the colour
chain per pixel and walks it back; ``augment_resize_normalize_backward`` is the VJP as a function).

Inference side (appv3.py ``detect_core``): ``View`` / ``detect_views`` + ``views_to_patch_operand`` build the app's 9 crops, its
90-degree rotated view and its 4 x 4 grid cells, 42 encoder rows per image, in one pass of ``sgl_op_preprocess_views``.
``views_resize_normalize(differentiable=True)`` is differentiable with respect to a float source (one
``sgl_op_preprocess_views_bwd``, the adjoint of all views at once; ``views_resize_normalize_backward`` is the VJP as a
function), which with ``heads.app_visual_prob`` gives the gradient of the app's visual probability in the source image.
``views_freq_features`` is the app's 24-D frequency / SRM vector (``extract_freq_vector``) of the crops and cells, one pass
of ``sgl_op_freq_features``; ``heads.app_freq_logits`` turns it into the ``z_freqs`` of ``core_signals_batched``.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import torch
import torch.nn as nn

from . import lib as _lib
from .config import get_config


@dataclass
class PatchOperand:
    """The patch GEMM's A operand [B*gh*gw, round_up(3*p*p, 64)] in the encoder's compute dtype, plus its geometry."""
    data: torch.Tensor
    batch: int
    height: int
    width: int


def _source(images: torch.Tensor):
    if not images.is_cuda:
        raise RuntimeError("the GPU input pipeline runs on CUDA tensors only (no CPU path)")
    if images.dtype == torch.uint8:
        if images.dim() != 4 or images.shape[-1] != 3:
            raise ValueError(f"uint8 images must be NHWC (B,H,W,3), got {tuple(images.shape)}")
        return images.contiguous(), 1, images.shape[0], images.shape[1], images.shape[2]
    if images.dim() != 4 or images.shape[1] != 3:
        raise ValueError(f"float images must be NCHW (B,3,H,W) in [0,1], got {tuple(images.shape)}")
    return images.float().contiguous(), 0, images.shape[0], images.shape[2], images.shape[3]


def _mix(mix_index, B, dev):
    if mix_index is None:
        return None
    idx = mix_index.to(device=dev, dtype=torch.int32).contiguous()
    if idx.numel() != B:
        raise ValueError("mix_index must have one entry per image")
    return idx


def _operand_dtype(compute_dtype: str) -> torch.dtype:
    """dtype of the patch-GEMM operand of an encoder in ``compute_dtype`` (strict modes read fp32)."""
    return {"bf16": torch.bfloat16, "fp16": torch.float16, "mxfp8": torch.bfloat16}.get(compute_dtype, torch.float32)


def _patch_geometry(config, size):
    """(S, (P, Kp)): the image side and the patch GEMM's patch size and padded K for ``config``."""
    cfg = get_config(config)
    P = cfg.patch_size
    return int(size or cfg.image_size), (P, (3 * P * P + 63) // 64 * 64)


def _alloc_out(n, size, patch, dtype, dev):
    """The output of ``n`` images or views and its ``(S, P, Kp, patch_major)`` arguments: ``patch`` None: the
    (n,3,size,size) image tensor; ``(P, Kp)``: the patch GEMM's operand rows."""
    if patch is None:
        return torch.empty((n, 3, size, size), device=dev, dtype=dtype), (size, 1, 3, 0)
    P, Kp = patch
    return torch.empty((n * (size // P) ** 2, Kp), device=dev, dtype=dtype), (size, P, Kp, 1)


def _grad_out(grad_out, rows: str) -> torch.Tensor:
    """``grad_out`` checked as a CUDA (``rows``,3,S,S) tensor: its detached fp32 contiguous form."""
    if not grad_out.is_cuda:
        raise RuntimeError("the GPU input pipeline runs on CUDA tensors only (no CPU path)")
    if grad_out.dim() != 4 or grad_out.shape[1] != 3 or grad_out.shape[2] != grad_out.shape[3]:
        raise ValueError(f"grad_out must be ({rows},3,S,S), got {tuple(grad_out.shape)}")
    return grad_out.detach().float().contiguous()


def _scratch(nbytes, dev):
    """``nbytes`` of device scratch, or None for none."""
    return torch.empty(nbytes, device=dev, dtype=torch.uint8) if nbytes else None


def _transform(images, size, patch, dtype, mean, std, mix_index=None, lam=1.0, params=None) -> torch.Tensor:
    """The one launch behind the four public transforms; ``patch`` as in ``_alloc_out``.  ``params`` None: sgl_op_preprocess
    (MixUp); a list of per-sample draws: sgl_op_preprocess_aug."""
    src, is_u8, B, Hs, Ws = _source(images)
    dev = src.device
    if params is not None and len(params) != B:
        raise ValueError("one augmentation record per image")
    out, layout = _alloc_out(B, size, patch, dtype, dev)
    common = (src.data_ptr(), is_u8, B, Hs, Ws, out.data_ptr(), _lib.dtype_code(dtype), *layout, float(mean), float(std))
    if params is None:
        idx = _mix(mix_index, B, dev)
        _lib.call("sgl_op_preprocess", dev, *common, _lib.ptr(idx), float(lam))
    else:
        tab = augment_table(params, dev)
        gm = torch.empty(B, device=dev, dtype=torch.float32)      # per-image means for the contrast operator
        _lib.call("sgl_op_preprocess_aug", dev, *common, tab.data_ptr(), gm.data_ptr())
    return out


def _wants_grad(images) -> bool:
    """A floating source that autograd would differentiate: the only case that leaves today's no-graph path."""
    return torch.is_grad_enabled() and images.is_floating_point() and images.requires_grad


def _refuse_grad(images, what: str, views: bool = False) -> None:
    """Everything but ``resize_normalize`` and the ``differentiable=True`` routes of ``views_resize_normalize`` and
    ``augment_resize_normalize`` has no backward: refuse rather than return a silently missing gradient.  ``views``: name the differentiable route of the view transforms."""
    if images.is_cuda and _wants_grad(images):
        if views:
            raise RuntimeError(
                f"{what} is not differentiable with respect to its source images as called (the patch-operand layout has "
                "no backward, and the NCHW views are differentiable only on request); use "
                "preprocess.views_resize_normalize(images, views, size, differentiable=True) and pass its result to the "
                "encoder as pixel_values=, or detach the images / run under torch.no_grad()")
        raise RuntimeError(
            f"{what} is not differentiable with respect to its source images as called (the patch-operand layout has no "
            "backward, and the augmenting transform is differentiable only on request); use "
            "preprocess.resize_normalize(images, size), which is, or preprocess.augment_resize_normalize(images, size, "
            "params, differentiable=True) / GpuTransform(..., differentiable=True), and pass the result to the encoder as "
            "pixel_values=, or detach the images / run under torch.no_grad()")


def resize_normalize_backward(grad_out: torch.Tensor, source_hw, mix_index: Optional[torch.Tensor] = None,
                              lam: float = 1.0, std: float = 0.5) -> torch.Tensor:
    """The vector-Jacobian product of ``resize_normalize`` as a function: ``grad_out`` (B,3,S,S) -> fp32 (B,3,Hs,Ws), the
    gradient with respect to a float source of size ``source_hw = (Hs, Ws)`` (for a uint8 source: with respect to
    ``bytes / 255``).  The transform is linear, so no source values are needed; one ``sgl_op_preprocess_bwd``, a gather with
    a fixed summation order: bitwise reproducible.  ``mix_index`` / ``lam`` / ``std`` as given to the forward."""
    g = _grad_out(grad_out, "B")
    B, S = g.shape[0], g.shape[2]
    Hs, Ws = int(source_hw[0]), int(source_hw[1])
    dev = g.device
    idx = _mix(mix_index, B, dev)
    d_src = torch.empty((B, 3, Hs, Ws), device=dev, dtype=torch.float32)
    nbytes = _lib.load().sgl_op_preprocess_bwd_scratch_bytes(B, Hs, Ws, S)
    scratch = _scratch(nbytes, dev)
    _lib.call("sgl_op_preprocess_bwd", dev, g.data_ptr(), B, Hs, Ws, S, float(std), _lib.ptr(idx), float(lam),
              d_src.data_ptr(), _lib.ptr(scratch), nbytes)
    return d_src


class _ResizeNormalize(torch.autograd.Function):
    """``resize_normalize`` for a source that requires grad: the same single forward launch, one
    ``sgl_op_preprocess_bwd`` backward.  Nothing is saved: the transform is linear in the source."""

    @staticmethod
    def forward(ctx, images, size, mean, std, mix_index, lam, dtype):
        ctx.src = (images.shape, images.dtype)
        ctx.args = (std, mix_index, lam)
        return _transform(images.detach(), size, None, dtype, mean, std, mix_index, lam)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        shape, src_dtype = ctx.src
        std, mix_index, lam = ctx.args
        d_src = resize_normalize_backward(grad_out, shape[2:], mix_index, lam, std)
        return d_src.to(src_dtype), None, None, None, None, None, None


def resize_normalize(images: torch.Tensor, size: int, mean: float = 0.5, std: float = 0.5,
                     mix_index: Optional[torch.Tensor] = None, lam: float = 1.0,
                     dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """(B,3,size,size) = Normalize(mean,std)(MixUp(Resize(size, antialias=True)(images))): the tensor the reference's GPU
    transform returns, in one pass.  Differentiable with respect to a floating ``images`` that requires grad (any float
    dtype, any strides): ``images.grad`` arrives in the source's dtype and shape; ``mix_index`` / ``lam`` get no gradient.
    uint8 sources have no gradient of their own: see ``resize_normalize_backward``."""
    if images.is_cuda and _wants_grad(images):
        return _ResizeNormalize.apply(images, size, mean, std, mix_index, lam, dtype)
    return _transform(images, size, None, dtype, mean, std, mix_index, lam)


def to_patch_operand(images: torch.Tensor, config, size: Optional[int] = None, compute_dtype: str = "bf16",
                     mean: float = 0.5, std: float = 0.5, mix_index: Optional[torch.Tensor] = None,
                     lam: float = 1.0) -> PatchOperand:
    """Resize (antialias) + MixUp + Normalize straight into the patch-embedding GEMM's operand for ``config`` (its patch
    size and K padding); feed the result to ``SiglipVisionModelHIP(patches=...)`` / ``encode_image(patches=...)``."""
    _refuse_grad(images, "to_patch_operand")
    S, patch = _patch_geometry(config, size)
    out = _transform(images, S, patch, _operand_dtype(compute_dtype), mean, std, mix_index, lam)
    return PatchOperand(out, images.shape[0], S, S)


# ---- augmentation branch (hidf_video_classifier.py:2868-2874) ----------------------------------------------------------
def sample_augmentation(batch: int, generator: Optional[torch.Generator] = None, p_flip: float = 0.5,
                        degrees: float = 5.0, p_rotation: float = 0.3, brightness: float = 0.1, contrast: float = 0.1,
                        saturation: float = 0.1, hue: float = 0.05, p_jitter: float = 0.3) -> list:
    """Host-side random draws of ``K.RandomHorizontalFlip(p=0.5)``, ``K.RandomRotation(degrees=5, p=0.3)`` and
    ``K.ColorJitter(0.1, 0.1, 0.1, 0.05, p=0.3)``: one dict per sample (the format ``augment_table`` packs and the oracle
    reads).  The RNG is the caller's ``torch.Generator``; nothing random happens on the device."""
    import math
    g = generator
    u = lambda n: torch.rand(n, generator=g)   # noqa: E731
    flip = u(batch) < p_flip
    rot = u(batch) < p_rotation
    ang = (u(batch) * 2 - 1) * degrees
    jit = u(batch) < p_jitter
    fb, fc, fs = (1 + (u(batch) * 2 - 1) * a for a in (brightness, contrast, saturation))
    fh = (u(batch) * 2 - 1) * hue
    out = []
    for b in range(batch):
        a = math.radians(float(ang[b])) if bool(rot[b]) else 0.0
        order = torch.randperm(4, generator=g).tolist() if bool(jit[b]) else None
        out.append(dict(flip=bool(flip[b]), cos=math.cos(a) if a else 1.0, sin=math.sin(a) if a else 0.0,
                        brightness=float(fb[b]), contrast=float(fc[b]), saturation=float(fs[b]), hue=float(fh[b]),
                        order=order))
    return out


def augment_table(params: list, device) -> torch.Tensor:
    """Pack per-sample parameters into the device table of ``sgl_aug_sample`` records (12 x 4 bytes each)."""
    import struct
    buf = bytearray()
    for pr in params:
        order = pr["order"] if pr["order"] else [-1, -1, -1, -1]
        buf += struct.pack("<7f5i", 1.0 if pr["flip"] else 0.0, pr["cos"], pr["sin"], pr["brightness"], pr["contrast"],
                           pr["saturation"], pr["hue"], *order, 0)
    return torch.frombuffer(buf, dtype=torch.uint8).to(device)


def augment_resize_normalize_backward(grad_out: torch.Tensor, images: torch.Tensor, params: list,
                                      std: float = 0.5) -> torch.Tensor:
    """The vector-Jacobian product of ``augment_resize_normalize`` as a function: ``grad_out`` (B,3,S,S) -> fp32
    (B,3,Hs,Ws), the gradient with respect to the source (for a uint8 NHWC source: with respect to ``bytes / 255``).  The
    colour chain is not linear, so the call takes the source ``images`` and the draws ``params`` the forward had; nothing
    else is kept: one ``sgl_op_preprocess_aug_bwd`` recomputes the chain per pixel and walks it back (clamps pass the
    gradient at their bounds, ties of max / min go to the lowest channel: ``torch.autograd``'s rules).  No atomics, a
    fixed summation order: bitwise reproducible."""
    g = _grad_out(grad_out, "B")
    src, is_u8, B, Hs, Ws = _source(images.detach())
    if src.device != g.device:
        raise ValueError("grad_out and images must live on the same device")
    if len(params) != B or g.shape[0] != B:
        raise ValueError("one augmentation record and one grad_out row per image")
    S = g.shape[2]
    dev = g.device
    tab = augment_table(params, dev)
    d_src = torch.empty((B, 3, Hs, Ws), device=dev, dtype=torch.float32)
    nbytes = _lib.load().sgl_op_preprocess_aug_bwd_scratch_bytes(B, Hs, Ws, S)
    scratch = _scratch(nbytes, dev)
    _lib.call("sgl_op_preprocess_aug_bwd", dev, g.data_ptr(), src.data_ptr(), is_u8, B, Hs, Ws, S, float(std),
              tab.data_ptr(), d_src.data_ptr(), _lib.ptr(scratch), nbytes)
    return d_src


class _AugmentResizeNormalize(torch.autograd.Function):
    """``augment_resize_normalize(differentiable=True)`` for a source that requires grad: the same forward launch, one
    ``sgl_op_preprocess_aug_bwd`` backward.  The source and the draws are kept (the chain is not linear; autograd refuses
    the backward if the source was modified in place in between); nothing else is saved."""

    @staticmethod
    def forward(ctx, images, size, params, mean, std, dtype):
        ctx.save_for_backward(images)
        ctx.args = (params, std)
        return _transform(images.detach(), size, None, dtype, mean, std, params=params)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        (images,) = ctx.saved_tensors
        params, std = ctx.args
        d_src = augment_resize_normalize_backward(grad_out, images.detach(), params, std)
        return d_src.to(images.dtype), None, None, None, None, None


def augment_resize_normalize(images: torch.Tensor, size: int, params: list, mean: float = 0.5, std: float = 0.5,
                             dtype: torch.dtype = torch.float32, differentiable: bool = False) -> torch.Tensor:
    """(B,3,size,size) = Normalize(ColorJitter(Rotation(Flip(Resize(images))))) with the given per-sample draws: the tensor
    the video trainer's augmenting GPU transform returns, in one pass over the pixels (plus a per-image mean pre-pass for
    the contrast operator).  ``differentiable=True`` makes it differentiable with respect to a floating ``images`` that
    requires grad (any float dtype, any strides; the same launch, so the same bits): ``images.grad`` arrives in the
    source's dtype, shape and strides; ``create_graph=True`` is not supported.  Without it such a source is refused, as
    before.  uint8 sources have no gradient of their own: see ``augment_resize_normalize_backward``."""
    if differentiable:
        params = list(params)
        if images.is_cuda and _wants_grad(images):
            return _AugmentResizeNormalize.apply(images, size, params, mean, std, dtype)
    else:
        _refuse_grad(images, "augment_resize_normalize")
    return _transform(images, size, None, dtype, mean, std, params=params)


def augment_to_patch_operand(images: torch.Tensor, config, params: list, size: Optional[int] = None,
                             compute_dtype: str = "bf16", mean: float = 0.5, std: float = 0.5) -> PatchOperand:
    """The augmenting transform written straight into the patch GEMM's operand (see ``to_patch_operand``)."""
    _refuse_grad(images, "augment_to_patch_operand")
    S, patch = _patch_geometry(config, size)
    out = _transform(images, S, patch, _operand_dtype(compute_dtype), mean, std, params=params)
    return PatchOperand(out, images.shape[0], S, S)


# ---- test-time views of the app (appv3.py:3214-3250 detect_core, :3315 make_multicrops, :3381 compute_patch_grid) ------
@dataclass(frozen=True)
class View:
    """One window onto source image ``src``: the half-open crop ``box = (x0, y0, x1, y1)`` (PIL's ``crop``), ``turns``
    counter-clockwise quarter turns (exact, extents swapping, or with ``keep_canvas`` what PIL's
    ``rotate(90 * turns)`` leaves on the crop's own canvas), then an optional left-right ``flip``.  The rules are in
    ``include/siglip_hip.h`` (``sgl_view``)."""
    src: int
    box: tuple
    turns: int = 0
    keep_canvas: bool = False
    flip: bool = False

    def oriented_hw(self):
        x0, y0, x1, y1 = self.box
        swap = self.turns % 2 == 1 and not self.keep_canvas
        return (x1 - x0, y1 - y0) if swap else (y1 - y0, x1 - x0)


def view_table(views, B: int, Hs: int, Ws: int):
    """Pack ``views`` into the host table of ``sgl_view`` records ``sgl_op_preprocess_views`` reads (a ctypes array), and
    raise ``ValueError`` for every record the C side would refuse as a bad shape."""
    views = list(views)
    if not views:
        raise ValueError("at least one view is needed")
    tab = (_lib.SglView * len(views))()
    for n, v in enumerate(views):
        if not isinstance(v, View):
            raise ValueError(f"view {n}: not a View: {v!r}")
        fields = (v.src, *v.box, v.turns, v.keep_canvas, v.flip)
        if len(v.box) != 4 or any(isinstance(f, float) or int(f) != f for f in fields):
            raise ValueError(f"view {n}: src, the four box coordinates and turns must be integers: {v!r}")
        x0, y0, x1, y1 = (int(t) for t in v.box)
        if not 0 <= v.src < B:
            raise ValueError(f"view {n}: src {v.src} outside the batch of {B}")
        if not (0 <= x0 < x1 <= Ws and 0 <= y0 < y1 <= Hs):
            raise ValueError(f"view {n}: box {tuple(v.box)} is empty or outside the {Ws} x {Hs} (w x h) source")
        if v.turns not in (0, 1, 2, 3):
            raise ValueError(f"view {n}: turns must be 0..3 (counter-clockwise quarter turns), got {v.turns}")
        if v.keep_canvas not in (0, 1) or v.flip not in (0, 1):
            raise ValueError(f"view {n}: keep_canvas and flip are flags")
        tab[n] = _lib.SglView(int(v.src), x0, y0, x1, y1, int(v.turns), int(v.keep_canvas), int(v.flip))
    return tab


def _views_transform(images, views, size, patch, dtype, mean, std) -> torch.Tensor:
    """The launches behind the two view transforms (one per 64 views): ``patch`` as in ``_alloc_out``."""
    src, is_u8, B, Hs, Ws = _source(images)
    dev = src.device
    tab = view_table(views, B, Hs, Ws)
    V = len(tab)
    out, layout = _alloc_out(V, size, patch, dtype, dev)
    nbytes = _lib.load().sgl_op_preprocess_views_scratch_bytes(V, size)
    scratch = _scratch(nbytes, dev)
    _lib.call("sgl_op_preprocess_views", dev, src.data_ptr(), is_u8, B, Hs, Ws, tab, V, out.data_ptr(),
              _lib.dtype_code(dtype), *layout, float(mean), float(std), _lib.ptr(scratch), nbytes)
    return out


def views_resize_normalize_backward(grad_out: torch.Tensor, views, source_shape, std: float = 0.5) -> torch.Tensor:
    """The vector-Jacobian product of ``views_resize_normalize`` as a function: ``grad_out`` (V,3,S,S) -> fp32 (B,3,Hs,Ws),
    the gradient with respect to float sources of ``source_shape = (B, Hs, Ws)`` (for uint8 sources: with respect to
    ``bytes / 255``), summed over the views of each source.  The transform is linear, so no source values are needed; one
    ``sgl_op_preprocess_views_bwd``, a gather with a fixed summation order: bitwise reproducible.  A source that no view
    names, and every pixel outside all boxes, gets exactly zero.  ``views`` / ``std`` as given to the forward."""
    g = _grad_out(grad_out, "V")
    B, Hs, Ws = (int(t) for t in source_shape)
    tab = view_table(views, B, Hs, Ws)
    V, S = len(tab), grad_out.shape[2]
    if grad_out.shape[0] != V:
        raise ValueError(f"grad_out has {grad_out.shape[0]} rows for {V} views")
    dev = g.device
    d_src = torch.empty((B, 3, Hs, Ws), device=dev, dtype=torch.float32)
    nbytes = _lib.load().sgl_op_preprocess_views_bwd_scratch_bytes(tab, V, S)
    scratch = _scratch(nbytes, dev)
    _lib.call("sgl_op_preprocess_views_bwd", dev, g.data_ptr(), B, Hs, Ws, tab, V, S, float(std), d_src.data_ptr(),
              _lib.ptr(scratch), nbytes)
    return d_src


class _ViewsResizeNormalize(torch.autograd.Function):
    """``views_resize_normalize(differentiable=True)`` for a source that requires grad: the same forward launches, one
    ``sgl_op_preprocess_views_bwd`` backward.  Nothing is saved: the transform is linear in the source."""

    @staticmethod
    def forward(ctx, images, views, size, mean, std, dtype):
        ctx.src = (images.shape, images.dtype)
        ctx.args = (views, std)
        return _views_transform(images.detach(), views, size, None, dtype, mean, std)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        shape, src_dtype = ctx.src
        views, std = ctx.args
        d_src = views_resize_normalize_backward(grad_out, views, (shape[0], shape[2], shape[3]), std)
        return d_src.to(src_dtype), None, None, None, None, None


def views_resize_normalize(images: torch.Tensor, views, size: int, mean: float = 0.5, std: float = 0.5,
                           dtype: torch.dtype = torch.float32, differentiable: bool = False) -> torch.Tensor:
    """(V,3,size,size): every ``View`` of the same-size sources ``images`` cropped, turned, mirrored, resized (antialias)
    and normalised in one pass: what the app builds per window with PIL ``crop`` / ``rotate`` and
    ``Resize -> ToTensor -> Normalize``.  ``differentiable=True`` makes it differentiable with respect to a floating
    ``images`` that requires grad (any float dtype, any strides; the same launches, so the same bits): ``images.grad``
    arrives in the source's dtype and shape, summed over all views.  Without it such a source is refused, as before.
    uint8 sources have no gradient of their own: see ``views_resize_normalize_backward``."""
    if differentiable:
        views = list(views)
        if images.is_cuda and _wants_grad(images):
            return _ViewsResizeNormalize.apply(images, views, size, mean, std, dtype)
    else:
        _refuse_grad(images, "views_resize_normalize", views=True)
    return _views_transform(images, views, size, None, dtype, mean, std)


def views_to_patch_operand(images: torch.Tensor, views, config, size: Optional[int] = None, compute_dtype: str = "bf16",
                           mean: float = 0.5, std: float = 0.5) -> PatchOperand:
    """The views written straight into the patch GEMM's operand (see ``to_patch_operand``): ``PatchOperand(batch=V)`` for
    ``SiglipVisionModelHIP(patches=...)`` / ``encode_image(patches=...)``, one encoder batch of V rows."""
    _refuse_grad(images, "views_to_patch_operand", views=True)
    S, patch = _patch_geometry(config, size)
    views = list(views)
    out = _views_transform(images, views, S, patch, _operand_dtype(compute_dtype), mean, std)
    return PatchOperand(out, len(views), S, S)


CROP_WEIGHTS = (0.20, 0.10, 0.10, 0.10, 0.10, 0.10, 0.10, 0.10, 0.10)


def multicrop_views(h: int, w: int, src: int = 0):
    """The app's 9-crop ensemble (``make_multicrops``, appv3.py:3315-3350) of an ``h x w`` image: centre (half size), left,
    right, top, bottom and the four quadrants, with the ``(9,)`` weights ``[0.20, 0.10 x 8]``.  For ``w < 4`` or ``h < 4``
    one full view with weight 1 (the app resizes that one bicubically: a stated deviation, this path has one filter)."""
    if w < 4 or h < 4:
        return [View(src, (0, 0, w, h))], torch.tensor([1.0])
    mw, mh = w // 2, h // 2
    cx0, cy0 = (w - mw) // 2, (h - mh) // 2
    boxes = [(cx0, cy0, cx0 + mw, cy0 + mh), (0, 0, mw, h), (w - mw, 0, w, h), (0, 0, w, mh), (0, h - mh, w, h),
             (0, 0, mw, mh), (w - mw, 0, w, mh), (0, h - mh, mw, h), (w - mw, h - mh, w, h)]
    return [View(src, b) for b in boxes], torch.tensor(CROP_WEIGHTS, dtype=torch.float32)


def rotated_view(box, src: int = 0) -> View:
    """The app's dual-view stabiliser input, ``pil.rotate(90, expand=False)`` of the window ``box`` (appv3.py:3241)."""
    return View(src, tuple(box), turns=1, keep_canvas=True)


def patch_grid_views(h: int, w: int, rows: int = 4, cols: int = 4, src: int = 0, min_side: int = 64) -> list:
    """The cell boxes of the app's heat-map grid (``compute_patch_grid``, appv3.py:3381-3405), row-major: cells of
    ``pw = max(8, w // cols)`` by ``ph = max(8, h // rows)``, the last row and column extended to the edge, an empty cell
    ``None``.  Below ``min_side`` (the app's MIN_SIDE) on either side the app computes no grid: ``[]``."""
    if w < min_side or h < min_side:
        return []
    pw, ph = max(8, w // cols), max(8, h // rows)
    out = []
    for r in range(rows):
        for c in range(cols):
            x0, y0 = c * pw, r * ph
            x1 = w if c == cols - 1 else min(w, x0 + pw)
            y1 = h if r == rows - 1 else min(h, y0 + ph)
            out.append(None if x1 <= x0 or y1 <= y0 else View(src, (x0, y0, x1, y1)))
    return out


@dataclass
class DetectViews:
    """The app's whole view set for one image, and where each family sits in it.  ``views[crops]`` are the multi-crop
    windows (``weights`` their ``(C,)`` weights), ``views[rot]`` the rotated full frame; grid cell ``n`` (row-major, empty
    cells skipped: ``cells`` lists the kept (row, col)) is ``views[grid_start + 2 n]`` followed by its rotated view."""
    views: list
    weights: torch.Tensor
    crops: slice
    rot: int
    grid_start: int
    cells: list

    @property
    def grid(self) -> slice:
        """The unrotated cell views."""
        return slice(self.grid_start, len(self.views), 2)

    @property
    def grid_rot(self) -> slice:
        """The cells' rotated views."""
        return slice(self.grid_start + 1, len(self.views), 2)

    @property
    def freq(self) -> list:
        """Indices of the views the app takes frequency features from (``extract_freq_vector``): ``crops``, then ``grid``."""
        return list(range(len(self.views))[self.crops]) + list(range(len(self.views))[self.grid])


def detect_views(h: int, w: int, grid=(4, 4), src: int = 0) -> DetectViews:
    """Everything ``detect_core`` + ``compute_patch_grid`` look at for one ``h x w`` image, as one list for one
    ``views_to_patch_operand`` call: the 9 crops, the rotated full frame, then every non-empty grid cell followed by its
    rotated view (9 + 1 + 2 * 16 = 42 encoder rows for the 4 x 4 grid).  With logits ``z`` (V,) of that batch:
    ``core_signals_batched(z[d.crops][None], d.weights, z_freqs, z[d.rot][None], ...)`` is the image's verdict and
    ``core_signals_batched(z[d.grid][:, None], ones(1), z_freqs_cells, z[d.grid_rot], ...)`` the cells' (multicrop=False),
    with ``z_freqs, z_freqs_cells = heads.app_freq_logits(images_u8, d, freq_mlp)`` (one ``views_freq_features`` pass over
    ``d.freq`` and one ``FreqMLPApp`` forward): all of ``detect_core`` stays on the device."""
    crops, weights = multicrop_views(h, w, src)
    views = list(crops)
    rot = len(views)
    views.append(rotated_view((0, 0, w, h), src))
    start = len(views)
    cells = []
    rows, cols = grid
    for n, cell in enumerate(patch_grid_views(h, w, rows, cols, src)):
        if cell is not None:
            cells.append((n // cols, n % cols))
            views += [cell, rotated_view(cell.box, src)]
    return DetectViews(views, weights, slice(0, rot), rot, start, cells)


# ---- the app's 24-D frequency / SRM feature vectors (appv3.py:1618-1728 extract_freq_vector) -----------------------------
FREQ_MAX_SIDE = 4096      # window side cap of sgl_op_freq_features (65 resize taps)


def _freq_tables():
    """The three (256, 256) uint8 index tables over the fftshift-ed plane, by the app's own torch calls and dtypes
    (``fft_features``, appv3.py:1640-1684): band 0..2, log-radius bucket 0..38, sector 0..7; 255 = member of none."""
    h = w = 256
    cy, cx = h // 2, w // 2
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    r = torch.sqrt((yy - cy) ** 2 + (xx - cx) ** 2)
    rmax = float(r.max())
    r1, r2 = 0.15 * rmax, 0.45 * rmax
    band = torch.full((h, w), 2, dtype=torch.uint8)
    band[(r > r1) & (r <= r2)] = 1
    band[r <= r1] = 0
    rb = torch.logspace(math.log10(1.0), math.log10(rmax + 1.0), 40)
    ridx = (torch.bucketize(r.flatten() + 1.0, rb) - 1).view(h, w)
    bucket = torch.where((ridx >= 0) & (ridx < 39), ridx, torch.full_like(ridx, 255)).to(torch.uint8)
    ang = torch.atan2(yy - cy, xx - cx)
    sector = torch.full((h, w), 255, dtype=torch.uint8)
    for n in range(8):
        a0 = -math.pi + n * (2 * math.pi / 8)            # numpy.linspace(-pi, pi, 8, endpoint=False)[n]: start + n * step
        sector[(ang >= a0) & (ang < a0 + math.pi / 4)] = n
    return band, bucket, sector


class FreqGeometry:
    """Owner of the index tables ``sgl_op_freq_features`` reduces against: built once on the host, uploaded once per
    device as one (3, 256, 256) uint8 tensor and kept for the process (192 KiB per device)."""

    def __init__(self):
        self._host = None
        self._device = {}

    def host(self):
        if self._host is None:
            self._host = _freq_tables()
        return self._host

    def on(self, device) -> torch.Tensor:
        key = torch.device(device)
        if key not in self._device:
            self._device[key] = torch.stack(self.host()).contiguous().to(key)
        return self._device[key]


_freq_geometry = FreqGeometry()


def freq_geometry():
    """``(band, bucket, sector)``: the (256, 256) uint8 masks of the spectral features over the fftshift-ed plane (centre
    (128, 128)): the radial band 0..2 (``r <= 0.15 rmax``, ``<= 0.45 rmax``, above), the log-radius bucket 0..38 of the
    slope fit and the 45-degree sector 0..7 of the anisotropy; 255 where a pixel belongs to none."""
    return _freq_geometry.host()


def freq_geometry_on(device) -> torch.Tensor:
    """The (3, 256, 256) uint8 device copy of ``freq_geometry()`` that ``sgl_op_freq_features`` takes as its ``geometry``
    argument: uploaded once per device and kept."""
    return _freq_geometry.on(device)


def views_freq_features(images_u8: torch.Tensor, views, standardize: bool = True, return_gray: bool = False):
    """(V, 24) float32: the app's frequency / SRM vector (``extract_freq_vector``: 7 spectral, 8 wavelet, 9 SRM values,
    standardised unless ``standardize=False``) of every plain ``View`` (a crop box; no turn, no flip) of the same-size uint8
    NHWC sources, in one ``sgl_op_freq_features`` pass.  ``return_gray=True`` also returns the (V, 256, 256) uint8 planes,
    bit for bit PIL's ``crop(box).convert("L").resize((256, 256), BICUBIC)``.  Inference only."""
    if _wants_grad(images_u8):
        raise ValueError("views_freq_features is not differentiable (integer gray plane, histogram); detach the source or "
                         "run under torch.no_grad(), and pass uint8 NHWC images")
    if images_u8.dtype != torch.uint8:
        raise ValueError(f"views_freq_features reads uint8 NHWC sources only (the app's PIL images), got {images_u8.dtype}; "
                         "convert with (images * 255).round().to(torch.uint8).permute(0, 2, 3, 1)")
    if images_u8.dim() != 4 or images_u8.shape[-1] != 3:
        raise ValueError(f"uint8 images must be NHWC (B,H,W,3), got {tuple(images_u8.shape)}")
    B, Hs, Ws = images_u8.shape[0], images_u8.shape[1], images_u8.shape[2]
    tab = view_table(views, B, Hs, Ws)
    for n, v in enumerate(tab):
        if v.turns or v.keep_canvas or v.flip:
            raise ValueError(f"view {n}: the frequency features are taken from unrotated, unmirrored windows only (as the "
                             "app does); pass View(src, box), and use views_resize_normalize for turned or flipped views")
        if v.x1 - v.x0 > FREQ_MAX_SIDE or v.y1 - v.y0 > FREQ_MAX_SIDE:
            raise ValueError(f"view {n}: window side above {FREQ_MAX_SIDE}; shrink the source first (the app's MAX_SIDE "
                             "pre-shrink) or split the window")
    src, _, B, Hs, Ws = _source(images_u8)
    dev = src.device
    V = len(tab)
    out = torch.empty((V, 24), device=dev, dtype=torch.float32)
    gray = torch.empty((V, 256, 256), device=dev, dtype=torch.uint8) if return_gray else None
    nbytes = _lib.load().sgl_op_freq_features_scratch_bytes(V, Hs, Ws)
    scratch = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    _lib.call("sgl_op_freq_features", dev, src.data_ptr(), B, Hs, Ws, tab, V, freq_geometry_on(dev).data_ptr(),
              out.data_ptr(), int(bool(standardize)), _lib.ptr(gray), scratch.data_ptr(), nbytes)
    return (out, gray) if return_gray else out


class GpuTransform(nn.Module):
    """``nn.Sequential(K.Resize(res, antialias=True), K.Normalize(0.5, 0.5))`` of the reference (cifake…:1791-1794,
    hidf_video_classifier.py:2874-2878) as one module; ``forward(images, mix_index=None, lam=1.0)``."""

    def __init__(self, resolution: int, mean: float = 0.5, std: float = 0.5, data_augmentation: bool = False,
                 generator: Optional[torch.Generator] = None, differentiable: bool = False):
        super().__init__()
        self.resolution, self.mean, self.std = int(resolution), float(mean), float(std)
        self.data_augmentation, self.generator = bool(data_augmentation), generator
        self.differentiable = bool(differentiable)

    def forward(self, images, mix_index=None, lam: float = 1.0):
        """``data_augmentation=True`` (hidf_video_classifier.py ``--data_augmentation``, :2866-2874) inserts flip / rotation /
        colour jitter between resize and normalize while the module is in training mode; draws come from ``generator``.
        The plain branch is differentiable with respect to floating ``images`` that require grad (``resize_normalize``);
        the augmentation branch refuses such a source unless the module was built with ``differentiable=True``
        (``augment_resize_normalize(differentiable=True)``).  The reference never puts its ``gpu_transform`` into eval mode, so
        with ``--data_augmentation`` it augments validation batches too.  This module augments only in training mode, on
        purpose: call ``.eval()`` for validation."""
        if self.data_augmentation and self.training:
            if not self.differentiable:
                _refuse_grad(images, "GpuTransform(data_augmentation=True) in training mode")
            if mix_index is not None:
                raise ValueError("MixUp and the augmentation branch belong to different trainers; use one of them")
            params = sample_augmentation(images.shape[0], self.generator)
            return augment_resize_normalize(images, self.resolution, params, self.mean, self.std,
                                            differentiable=self.differentiable)
        return resize_normalize(images, self.resolution, self.mean, self.std, mix_index, lam)
